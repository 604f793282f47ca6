"""Which level body each wave of a shared hand-off group launch runs
(csrc/kernels/jacobi5tb.hpp tb_block: the `rule_kind` block), from the
kernel's own constants (ops.jacobi5tb_shared_geom / gmt_jacobi5tb_shared_geom)
and plain arithmetic, and the case lists of tests/test_tb_shared_rules_gpu.py,
so the CPU suite can assert what the GPU cases reach
(tests/test_tb_shared_model.py).

The model predicts; the kernel decides.  Coordinates are array columns / rows;
rect and dom are (x0, nx, y0, ny) as in ops.jacobi5tb; mask bits 1 W, 2 E,
4 S, 8 N mark halo sides (clear: a fixed Dirichlet ring)."""
from collections import namedtuple

COLS = 256  # columns of a wave's window
KS = (12, 16, 20)
STRIPS = (4, 2)

# kind: "plain" | "general" | "keep"; slot: the ghost column's lane slot (keep,
# and general by slot); side: "W" / "E" ghost held by the window ("WE" both,
# "" none); cause (general only): "row" a fixed row in the segment's cone,
# "both" two ghost columns, "slot" one ghost column in a slot without a body,
# "col" fixed columns but no ghost column in the window
Wave = namedtuple("Wave", "gi sl stage seg cf kind slot side cause")


def group_starts(geom, rect):
    """First output column of every group: GOUT apart, the last one shifted
    left to end at the rect's edge."""
    rx0, nx = rect[0], rect[1]
    assert nx >= geom["GOUT"], "a shared launch needs a rect at least one group wide"
    n = -(-nx // geom["GOUT"])
    return [min(rx0 + gi * geom["GOUT"], rx0 + nx - geom["GOUT"]) for gi in range(n)]


def window_start(geom, gx, sl, stage):
    ga = gx - geom["ML"]
    return ga + geom["S0"] * sl if stage == 0 else ga + geom["O"] + geom["S1"] * sl


def segments(rect, seg_rows):
    """[ys, ye) of every segment: one for a short rect with the default
    planner, tb_block's even split of ceil(ny / seg_rows) segments otherwise."""
    y0, ny = rect[2], rect[3]
    if seg_rows == 0:
        assert ny <= 128, "the default planner's segments are not modelled above 128 rows"
        return [(y0, y0 + ny)]
    nm = -(-ny // seg_rows)
    return [(y0 + m * ny // nm, y0 + (m + 1) * ny // nm) for m in range(nm)]


def wave_body(k, geom, cf, ys, ye, dom, mask):
    """(kind, slot, side, cause) of a wave whose window starts at column cf,
    on segment rows [ys, ye)."""
    dx0, dnx, dy0, dny = dom
    cx0, cx1 = cf, cf + COLS
    ry = (ys - k < dy0 and not mask & 4) or (ye + k > dy0 + dny and not mask & 8)
    rule = (cx0 < dx0 and not mask & 1) or (cx1 > dx0 + dnx and not mask & 2) or ry
    gw0, ge0 = dx0 - 1, dx0 + dnx
    hw = not mask & 1 and cx0 <= gw0 < cx1
    he = not mask & 2 and cx0 <= ge0 < cx1
    side = ("W" if hw else "") + ("E" if he else "")
    if not rule:
        return "plain", None, side, None
    if ry:
        return "general", None, side, "row"
    if hw and he:
        return "general", None, side, "both"
    if not hw and not he:
        return "general", None, side, "col"
    slot = ((gw0 if hw else ge0) - cx0) & 3
    if slot in (geom["kJW"], geom["kJE"]):
        return "keep", slot, side, None
    return "general", slot, side, "slot"


def waves(k, strips, geom, rect, dom, mask, seg_rows=0):
    """Every (group, strip, stage, segment) wave of the launch with its body."""
    out = []
    for gi, gx in enumerate(group_starts(geom, rect)):
        for sl in range(strips):
            for stage in (0, 1):
                cf = window_start(geom, gx, sl, stage)
                for m, (ys, ye) in enumerate(segments(rect, seg_rows)):
                    out.append(Wave(gi, sl, stage, m, cf, *wave_body(k, geom, cf, ys, ye, dom, mask)))
    return out


def ghost_in_window(geom, strips, rect, dom, side):
    """True if some wave's window holds the `side` ghost column of dom."""
    g = dom[0] - 1 if side == "W" else dom[0] + dom[1]
    return any(0 <= g - window_start(geom, gx, sl, st) < COLS
               for gx in group_starts(geom, rect) for sl in range(strips) for st in (0, 1))


def max_inset(geom, strips, side, nx=None):
    """The largest inset d of a rect (nx wide, default two groups and 37
    columns) from the domain's `side` edge at which a window still holds
    that side's ghost column (found by search: the windows of a group are
    contiguous, so the ghost leaves them once)."""
    nx = 2 * geom["GOUT"] + 37 if nx is None else nx
    d = 0
    while ghost_in_window(geom, strips, (1000, nx, 0, 1), (1000 - (d if side == "W" else 0), nx + d, 0, 1), side):
        d += 1
        assert d < 2 * COLS
    return d - 1


# ---- the case lists of tests/test_tb_shared_rules_gpu.py ----
# Keys are plain tuples (no geometry: test ids need no library); a Case is a
# key resolved with the query's constants.

NY_A, NY_B, SEG_B = 45, 200, 64
Case = namedtuple("Case", "k strips exact side d mask ncol rect dom seg_rows")

# A: one-column keeps, one segment.  Insets of the rect from the domain's
# ghost side: 0-3 (every lane slot), NL, the largest with the ghost column
# still in a window ("max") and one more ("out": no keep on that side);
# insets_a(k)'s two (stage 0 alone holds the ghost, in either slot);
# "tight": d = 0 with the smallest margins the ABI allows, so windows
# overhang both ends of a row; side "WE": both x sides Dirichlet, one group.
INSETS_A = ("0", "1", "2", "3", "NL", "max", "out", "tight")


def insets_a(k):
    """INSETS_A and the smallest insets >= NL = k / 2 that are 0 and 3 mod 4:
    the stage-1 windows no longer hold the ghost column, the stage-0 window
    holds it in the side's own slot / the other side's slot."""
    nl = k // 2
    more = [str(d) for d in ((nl + 3) // 4 * 4, nl + (3 - nl) % 4) if d != nl]
    return INSETS_A + tuple(more)


KEYS_A = [(k, strips, exact, side, sel) for k in KS for strips in STRIPS for exact in (False, True)
          for side in "WE" for sel in insets_a(k)] + \
         [(k, strips, exact, "WE", "0") for k in KS for strips in STRIPS for exact in (False, True)]
# B: fixed-row and one-column bodies in one launch (four 50-row segments)
KEYS_B = [(k, strips, exact, side) for k in KS for strips in STRIPS for exact in (False, True)
          for side in ("", "W", "E")]
# D: the engine's core + frame launches, the core rect (inset K on its halo
# sides) at least one four-strip group wide: nx = GOUT + 2 K + dw
MASKS_D, NY_D, DW_D = (15, 3, 7, 11), 90, (0, 1, 5)


def inset(dom, side, d):
    x0, nx, y0, ny = dom
    return (x0 + d, nx - d, y0, ny) if side == "W" else (x0, nx - d, y0, ny)


def case_a(key, geom):
    k, strips, exact, side, sel = key
    if side == "WE":
        dom = (24, geom["GOUT"], k, NY_A)
        return Case(k, strips, exact, side, 0, 12, 24 + geom["GOUT"] + k + 3, dom, dom, 0)
    nx = 2 * geom["GOUT"] + 37  # three groups: the last one shifted, the middle one plain
    d = {"NL": geom["NL"], "max": max_inset(geom, strips, side, nx), "out": max_inset(geom, strips, side, nx) + 1,
         "tight": 0}.get(sel)
    d = int(sel) if d is None else d
    xo = k if sel == "tight" else 24 + d % 2
    dom = (xo, nx + d, k, NY_A)
    ncol = xo + nx + d + (k if sel == "tight" else k + 3)
    return Case(k, strips, exact, side, d, 14 if side == "W" else 13, ncol, inset(dom, side, d), dom, 0)


def case_b(key, geom):
    k, strips, exact, side = key
    dom = (24, 2 * geom["GOUT"] + 37, k, NY_B)
    d = 3 if side else 0
    return Case(k, strips, exact, side, d, 0, 24 + dom[1] + k + 3, inset(dom, side, d) if side else dom, dom, SEG_B)


def case_waves(c, geom):
    return waves(c.k, c.strips, geom, c.rect, c.dom, c.mask, c.seg_rows)


def nx_d(k, dw, geom4):
    return geom4["GOUT"] + 2 * k + dw
