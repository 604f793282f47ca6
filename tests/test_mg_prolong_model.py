"""engine.mg_prolong_levels (the Python model of the rule of
mg(fuse_prolong=True)) against tables derived by hand from the share rule, and
against what the engine reports (CPU backend).

A level fuses iff nu2 >= 1, its transfer is not table-driven, and there is one
rank or every rank owns c/2 + 1 cells of the next coarser level on each shared
axis, c = min(n2, depth), n2 = nu2 sweeps or 2 nu2 half-sweeps.

9 x 9 on a (2, 1) grid: the levels are 9 x 9 and 4 x 4; the process rows own
5 / 4 fine rows (depth 4 with a ghost depth of 4) and 2 / 2 coarse rows.  c = 4
needs 3 coarse rows a rank: not fused; c = 2 or 3 needs 2: fused.

255 x 767 on (2, 1): rows 128/127, 64/63, 32/31, 16/15, 8/7, 4/3, 2/1 (see
tests/test_mg_fuse_model.py), depths [4, 4, 4, 4, 4, 3] at fuse = 4.  The
7-row level (5) interpolates from the 3-row one, whose shares are 2 / 1: it
fuses only with c = 1."""
import pytest

from test_mg_cpu import launch_cpu


def test_levels_by_hand():
    from gpu_mpi_tests_amd import engine

    p = engine.mg_prolong_levels
    assert engine.mg_levels(9, 9, (2, 1)) == [(9, 9), (4, 4)]
    assert engine.mg_fuse_depths(9, 9, (2, 1), 4, 4) == [4]
    assert p(9, 9, (2, 1), 4, 4, 2, "rb") == []             # depth 4, n2 = 4: c = 4 needs 3 coarse rows, there are 2
    assert p(9, 9, (2, 1), 4, 4, 4, "jacobi") == []         # the same c from four Jacobi sweeps
    assert p(9, 9, (2, 1), 4, 4, 2, "jacobi") == [0]        # c = 2 needs 2
    assert p(9, 9, (2, 1), 4, 4, 3, "jacobi") == [0]        # c = 3 needs 2
    assert p(9, 9, (2, 1), 4, 2, 2, "rb") == [0]            # fuse = 2: depth 2, c = 2
    assert p(9, 9, (2, 1), 2, 4, 2, "rb") == [0]            # ghost depth 2 caps level 0: c = 2
    assert p(9, 9, (1, 2), 4, 4, 2, "rb") == []             # the same shares along x
    assert p(9, 9, (1, 1), 1, 4, 2, "rb") == [0]            # one rank: no share to ask for
    # nu2 = 0: no post-smoothing pass to fuse into
    assert p(9, 9, (1, 1), 4, 4, 0, "jacobi") == [] and p(255, 767, (2, 1), 4, 4, 0, "rb") == []
    # 255 x 767 on (2, 1)
    assert p(255, 767, (2, 1), 4, 4, 2, "rb") == [0, 1, 2, 3, 4]     # level 4: c = 4, coarse shares 4 / 3
    assert p(255, 767, (2, 1), 4, 4, 2, "jacobi") == [0, 1, 2, 3, 4]  # level 5: c = 2 needs 2 rows, a rank has 1
    assert p(255, 767, (2, 1), 4, 4, 1, "jacobi") == [0, 1, 2, 3, 4, 5]  # c = 1 needs 1
    assert p(255, 767, (2, 1), 4, 0, 2, "jacobi") == [0, 1, 2, 3, 4, 5]  # fuse = 0: depth 1 everywhere, c = 1
    assert p(255, 767, (1, 1), 1, 4, 2, "rb") == [0, 1, 2, 3, 4, 5, 6]   # one rank: every level
    assert p(255, 767, (2, 1), 4, 4, 2, "rb", 3) == [0, 1]               # max_levels = 3
    # coarsen = "any": 64 x 64 -> 31 x 31 goes by tables, the nested levels below it fuse
    table = engine.mg_levels(64, 64, (1, 1), 0, "any")
    assert table[:2] == [(64, 64), (31, 31)]
    assert p(64, 64, (1, 1), 2, 2, 2, "jacobi", 0, "any") == list(range(1, len(table) - 1))
    assert 0 not in p(64, 64, (2, 2), 2, 2, 2, "rb", 0, "any")
    with pytest.raises(ValueError):
        p(9, 9, (1, 1), 1, 0, 2, "sor")


@pytest.mark.parametrize("np_,dims", [(1, None), (2, (2, 1))], ids=lambda v: None if isinstance(v, int) else str(v))
def test_engine_reports_the_model(np_, dims):
    """9 x 9 with tsteps = 4: the C++ rule inside the engine gives the model's levels, c = 4 included."""
    from gpu_mpi_tests_amd import engine

    cases = [(fuse, nu2, sm) for fuse in (0, 2, 4) for nu2 in (0, 1, 2, 4) for sm in ("jacobi", "rb")]
    ops = [dict(op="mg", kw=dict(max_cycles=1, fuse=fuse, nu=(1, nu2), smoother=sm, fuse_prolong=True))
           for fuse, nu2, sm in cases]
    res = launch_cpu(dict(ny=9, nx=9, dims=dims, tsteps=4, ops=ops), np_)
    seen = set()
    for (fuse, nu2, sm), r in zip(cases, res[1:]):
        want = engine.mg_prolong_levels(9, 9, dims or (1, 1), 4, fuse, nu2, sm)
        assert r["same"] and r["res"]["fuse_prolong"] is True and r["res"]["prolong_levels"] == want, (fuse, nu2, sm, r)
        seen.add(tuple(want))
    assert seen == {(), (0,)}
