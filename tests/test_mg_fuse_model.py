"""engine.mg_fuse_depths (the Python model of the depth rule of mg(fuse=...))
against tables derived by hand from the share rule, and against what the engine
reports (CPU backend).

255 x 767 on a (2, 1) grid: the levels have 255, 127, 63, 31, 15, 7 and 3 rows;
a rank owning fine rows [oy, oy + n) owns coarse rows [oy/2, (oy + n)/2), so the
two process rows own 128/127, 64/63, 32/31, 16/15, 8/7, 4/3 and 2/1 rows.  The
coarsest (3-row) level does not smooth.  The 7-row level has shares 4 / 3: depth
3 at fuse = 4 (and 3), 2 at fuse = 2.  A ghost depth of 1 caps level 0 at 1 on
any grid of several ranks and not at all on one rank."""
import pytest

from test_mg_cpu import launch_cpu


def test_depths_by_hand():
    from gpu_mpi_tests_amd import engine

    d = engine.mg_fuse_depths
    assert [n for n, _ in engine.mg_levels(255, 767, (2, 1))] == [255, 127, 63, 31, 15, 7, 3]
    assert d(255, 767, (2, 1), 4, 4) == [4, 4, 4, 4, 4, 3]
    assert d(255, 767, (2, 1), 3, 4) == [3, 3, 3, 3, 3, 3]
    assert d(255, 767, (2, 1), 2, 4) == [2, 2, 2, 2, 2, 2]
    assert d(255, 767, (2, 1), 4, 1) == [1, 4, 4, 4, 4, 3]       # the ghost depth caps level 0 only
    assert d(255, 767, (2, 1), 4, 2) == [2, 4, 4, 4, 4, 3]
    assert d(255, 767, (2, 1), 4, 20) == [4, 4, 4, 4, 4, 3]
    assert d(255, 767, (2, 1), 0, 4) == [1] * 6                  # off
    # one rank: every side is a ring side, no ghost depth is needed, every level fuses (eight levels down to 1 x 5)
    assert d(255, 767, (1, 1), 4, 1) == [4] * 7
    # columns only: 767 -> 383 -> 191 -> 95 -> 47 -> 23 -> 11 -> 5 over two ranks; 11 columns are 5 / 6
    assert d(255, 767, (1, 2), 4, 4) == [4] * 7
    # three process columns: 23 columns are 7 / 8 / 8, 11 are 3 / 4 / 4 (the coarsest here: two process rows)
    assert d(255, 767, (2, 3), 4, 4) == [4, 4, 4, 4, 4, 3]
    # max_levels = 3: two smoothing levels
    assert d(255, 767, (2, 1), 4, 1, 3) == [1, 4]
    # 15 x 15 on (4, 1): rows 4/4/4/3 -> 2/2/2/1 (7 rows) -> the 3-row level would leave a rank without a row
    assert engine.mg_levels(15, 15, (4, 1)) == [(15, 15), (7, 7)]
    assert d(15, 15, (4, 1), 4, 4) == [3]
    assert d(31, 31, (4, 1), 4, 4) == [4, 3]                     # 8/8/8/7, then 4/4/4/3; 7 rows 2/2/2/1 is the coarsest
    # any size: 256 x 768 -> 127 x 383 -> ... as the nested table from there
    assert d(256, 768, (2, 1), 4, 4, 0, "any")[:2] == [4, 4]
    assert len(d(256, 768, (2, 1), 4, 4, 0, "any")) == len(engine.mg_levels(256, 768, (2, 1), 0, "any")) - 1


@pytest.mark.parametrize("np_,dims,tsteps", [(1, None, 1), (2, (2, 1), 1), (2, (2, 1), 4), (4, (2, 2), 2)],
                         ids=lambda v: None if isinstance(v, int) else str(v))
def test_engine_reports_the_model(np_, dims, tsteps):
    from gpu_mpi_tests_amd import engine

    cases = [(fuse, ml) for fuse in (2, 3, 4) for ml in (0, 3)]
    ops = [dict(op="mg", kw=dict(max_cycles=1, fuse=fuse, max_levels=ml)) for fuse, ml in cases]
    res = launch_cpu(dict(ny=255, nx=767, dims=dims, tsteps=tsteps, ops=ops), np_)
    for (fuse, ml), r in zip(cases, res[1:]):
        depths = engine.mg_fuse_depths(255, 767, dims or (1, 1), fuse, tsteps, ml)
        got = r["res"]
        assert r["same"] and got["fuse"] == fuse, got
        assert (got["fuse_fine"], got["fuse_levels"]) == (depths[0], sum(x >= 2 for x in depths)), (fuse, ml, got, depths)
