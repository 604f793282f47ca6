"""The derived bounds of tests/kernel_refs.py hold for the plain fp64 torch
references (ops/reference.py) on every shape the GPU path tests use: a check
of the bound helper itself, on the CPU."""
import torch

import kernel_refs as kr
from gpu_mpi_tests_amd.ops import reference as ref


def test_fp64_references_within_derived_bounds():
    for dim, cases in ((1, kr.WIN_CASES + kr.DMA_CASES + kr.LONG_CASES + kr.PT1_CASES), (0, kr.PT0_CASES)):
        for ny, nx in cases:
            for default in (False, True) if (dim, ny, nx) in kr.DEFAULT_COEF_CASES else (False,):
                z, r, bound, coef, scale = kr.stencil_case(dim, ny, nx, default)
                kr.check(ref.stencil5_2d(z, dim, scale, coef), r, bound, f"stencil5_2d dim {dim} {ny}x{nx}")
    for n in kr.ONE_D_CASES:
        z, r, bound, coef, scale = kr.stencil_case(None, 1, n)
        kr.check(ref.stencil5_1d(z, scale, coef), r, bound, f"stencil5_1d {n}")
    for ny, nx in kr.REDUCE_CASES:
        a, b = kr.reduce_case(ny, nx)
        for keep in (0, 1):
            kr.check(ref.sum_axis(a, keep), *kr.sum_ref(a, 0 if keep == 0 else 1), f"sum_axis keep {keep} {ny}x{nx}")
        kr.check(ref.diff_sq(a, b), *kr.diff_sq_ref(a, b), f"diff_sq {ny}x{nx}")


def test_field_values():
    """The inputs are what the bounds assume: magnitudes in [2^-9, 2^8), both
    signs; for the reductions in [0.5, 1)."""
    z = kr.field((64, 257), seed=1)
    assert float(z.abs().min()) >= 2.0 ** -9 and float(z.abs().max()) <= 2.0 ** 8
    assert bool((z > 0).any()) and bool((z < 0).any())
    s = kr.field((64, 257), seed=1, emax=0)
    assert float(s.abs().min()) >= 0.5 and float(s.abs().max()) <= 1.0
    assert torch.equal(z, kr.field((64, 257), seed=1))


def test_host_backend_answers_path_none():
    """The CPU backend exports the path queries of gmt/kernels.h (same ABI)
    and has no kernel to name.  In a child process: the library shares its
    SONAME with the GPU one."""
    import os
    import subprocess
    import sys
    lib = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "build", "lib-host", "libgmt.so")
    code = ("import ctypes, sys; L = ctypes.CDLL(sys.argv[1]); s = ctypes.c_int64(7); i = ctypes.c_int64;"
            "print(L.gmt_stencil5_2d_path(1, i(257), i(133), None, i(258), None, i(258), ctypes.byref(s)), s.value,"
            " L.gmt_jacobi5_path(i(8), None, None, i(64), None, i(0)))")
    p = subprocess.run([sys.executable, "-c", code, lib], capture_output=True, text=True, timeout=60, check=True)
    assert p.stdout.split() == ["0", "0", "0"]


def test_check_rejects_one_lost_element():
    """kr.check fires when one element of a row sum is dropped (the kind of
    slip the path tests are after)."""
    import pytest
    a, _ = kr.reduce_case(17, 4097)
    r, bound = kr.sum_ref(a, 1)
    with pytest.raises(AssertionError):
        kr.check(a[:, :-1].sum(dim=1), r, bound, "row sums without the last column")
    t, tb = kr.sum_ref(a, None)  # a single number is checked like an array
    kr.check(a.sum(), t, tb, "total")
    with pytest.raises(AssertionError):
        kr.check(a.sum() - a[3, 5], t, tb, "total without one element")
