"""CPU side of tests/test_tb_shared_rules_gpu.py: the shared-group geometry
query (gmt_jacobi5tb_shared_geom, here from the CPU backend: one header,
gmt/tb_geom.h, serves both), what the GPU cases reach according to the model
(tests/tb_shared_model.py), and the reference on inset rects."""
import functools
import json
import os
import subprocess
import sys

import torch

import tb_shared_model as tm
from gpu_mpi_tests_amd.ops import reference as ref
from test_jacobi_tb_gpu import _engine_frame

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_LIB = os.path.join(ROOT, "build", "lib-host", "libgmt.so")
NAMES = ("GOUT", "ML", "NL", "O", "S0", "S1", "kJW", "kJE")
# documented values (csrc/include/gmt/kernels.h gmt_tb_opts.shared, README)
GOUT = {(12, 4): 952, (16, 4): 936, (20, 4): 920, (12, 2): 472, (16, 2): 464, (20, 2): 448}


@functools.lru_cache(maxsize=None)
def _query():
    """{(k, strips): (return code, the 8 values)} from the CPU backend, in a
    child process (the library shares its SONAME with the GPU one)."""
    code = ("import ctypes, json, sys; L = ctypes.CDLL(sys.argv[1]); r = {}\n"
            "for k in range(0, 26):\n"
            "    for s in (1, 2, 3, 4, 8):\n"
            "        o = (ctypes.c_int64 * 8)(*([-1] * 8))\n"
            "        r['%d,%d' % (k, s)] = [L.gmt_jacobi5tb_shared_geom(k, s, o), list(o)]\n"
            "r['null'] = L.gmt_jacobi5tb_shared_geom(20, 4, None)\n"
            "print(json.dumps(r))")
    p = subprocess.run([sys.executable, "-c", code, HOST_LIB], capture_output=True, text=True, timeout=60, check=True)
    return json.loads(p.stdout)


def _geoms():
    q = _query()
    return {(k, s): dict(zip(NAMES, q[f"{k},{s}"][1])) for k in tm.KS for s in tm.STRIPS}


def test_geometry_query():
    q = _query()
    assert q.pop("null") != 0
    for key, (rc, vals) in q.items():
        k, s = (int(v) for v in key.split(","))
        if k in tm.KS and s in tm.STRIPS:
            assert rc == 0, key
            g = dict(zip(NAMES, vals))
            assert g["GOUT"] == GOUT[k, s]
            assert g["NL"] == k // 2 and g["ML"] == g["O"] + g["NL"] and g["O"] % 4 == 0 and g["O"] >= g["NL"]
            assert g["kJW"] == (g["ML"] - 1) % 4 and g["kJE"] == (g["GOUT"] + g["ML"]) % 4
            assert g["kJW"] != g["kJE"]
            assert g["S0"] == 256 - 2 * g["NL"] and g["S1"] % 4 == 0 and 0 < g["S1"] <= g["S0"]
            assert g["GOUT"] == g["S1"] * (s - 1) + 256 - 2 * g["NL"]
            # the last stage-1 window ends inside the group's valid level-NL columns
            assert g["O"] + g["S1"] * (s - 1) + 256 <= g["S0"] * (s - 1) + 256 - g["NL"]
        else:
            assert rc != 0 and vals == [-1] * 8, key  # no group kernel: nothing written
    g = _geoms()
    assert [(g[k, 4]["kJW"], g[k, 4]["kJE"]) for k in tm.KS] == [(1, 2), (3, 0), (1, 2)]


def test_model_windows():
    """The model's windows tile a group as the kernel's comment says: the
    stage-0 windows' valid columns abut, the stage-1 outputs tile GOUT."""
    for (k, s), g in _geoms().items():
        gx = 1000
        w0 = [tm.window_start(g, gx, sl, 0) for sl in range(s)]
        w1 = [tm.window_start(g, gx, sl, 1) for sl in range(s)]
        assert all(b + g["NL"] == a + 256 - g["NL"] for a, b in zip(w0, w0[1:]))
        assert w1[0] + g["NL"] == gx and w1[-1] + 256 - g["NL"] == gx + g["GOUT"]
        assert all(b - a <= 256 - 2 * g["NL"] for a, b in zip(w1, w1[1:]))
        # groups: GOUT apart, the last one shifted left to the rect's edge
        assert tm.group_starts(g, (50, 2 * g["GOUT"] + 37, 0, 1)) == [50, 50 + g["GOUT"], 50 + g["GOUT"] + 37]
        assert tm.group_starts(g, (50, g["GOUT"], 0, 1)) == [50]
    assert tm.segments((0, 1, 20, 200), 64) == [(20, 70), (70, 120), (120, 170), (170, 220)]
    assert tm.segments((0, 1, 20, 45), 0) == [(20, 65)]


def test_cases_reach_every_body():
    """Over the case lists A and B, for every (K, group width, exact): both
    one-column slots in both stages and with both ghost sides, the general
    body by slot and by fixed row, the plain body, and a ghost column held
    by stage 0 alone."""
    geoms = _geoms()
    for k in tm.KS:
        for strips in tm.STRIPS:
            g = geoms[k, strips]
            for exact in (False, True):
                cases = [tm.case_a(key, g) for key in tm.KEYS_A if key[:3] == (k, strips, exact)]
                cases += [tm.case_b(key, g) for key in tm.KEYS_B if key[:3] == (k, strips, exact)]
                assert len(cases) == 2 * len(tm.insets_a(k)) + 1 + 3
                keeps, sides, general, plain, stage0_only = set(), set(), set(), False, False
                for c in cases:
                    ws = tm.case_waves(c, g)
                    for w in ws:
                        if w.kind == "keep":
                            keeps.add((w.slot, w.stage))
                            sides.add((w.slot, w.side))
                        elif w.kind == "general":
                            general.add(w.cause)
                        else:
                            plain = True
                    for side in "WE":
                        held = {w.stage for w in ws if side in w.side}
                        stage0_only |= held == {0}
                tag = (k, strips, exact)
                assert keeps == {(s, st) for s in (g["kJW"], g["kJE"]) for st in (0, 1)}, tag
                assert sides == {(s, sd) for s in (g["kJW"], g["kJE"]) for sd in "WE"}, tag
                assert {"slot", "row"} <= general, tag
                assert plain and stage0_only, tag


def test_cases_inset_slots():
    """rect = dom puts the W ghost in slot kJW and the E ghost in kJE; an
    inset of 3 swaps them; insets 1 and 2 leave the one-column bodies; past
    the largest inset no wave holds the ghost column."""
    geoms = _geoms()
    for k, strips, exact, side, sel in tm.KEYS_A:
        if exact or side == "WE":
            continue
        g = geoms[k, strips]
        c = tm.case_a((k, strips, exact, side, sel), g)
        ws = [w for w in tm.case_waves(c, g) if side in w.side]
        own, other = (g["kJW"], g["kJE"]) if side == "W" else (g["kJE"], g["kJW"])
        if sel in ("0", "tight"):
            assert ws and all(w.kind == "keep" and w.slot == own for w in ws)
            assert {w.stage for w in ws} == {0, 1}
        elif sel == "3":
            assert ws and all(w.kind == "keep" and w.slot == other for w in ws)
            assert {w.stage for w in ws} == {0, 1}
        elif sel.isdigit() and int(sel) >= g["NL"]:
            assert [(w.kind, w.stage) for w in ws] == [("keep", 0)]
            assert ws[0].slot == (own if int(sel) % 4 == 0 else other)
        elif sel == "max":
            assert ws and {w.stage for w in ws} == {0}
        elif sel == "out":
            assert not ws and all(w.kind != "keep" for w in tm.case_waves(c, g))
        # every array holds the K-wide ring of its rect (the ABI's condition)
        assert c.rect[0] >= k and c.rect[0] + c.rect[1] + k <= c.ncol
        if sel == "tight":
            assert c.rect[0] == k and c.rect[0] + c.rect[1] + k == c.ncol


def _ref(k, h, rects, dom, mask):
    out = torch.full(h.shape, 7.0, dtype=torch.float64)
    ref.jacobi5xk(k, h, out, rects, dom, mask)
    return out


def _assert_rect_of(part, whole, rects):
    """`part` equals `whole` inside the rects and is untouched outside."""
    inside = torch.zeros(part.shape, dtype=torch.bool)
    for x0, nx, y0, ny in rects:
        inside[y0:y0 + ny, x0:x0 + nx] = True
    assert torch.equal(part[inside], whole[inside])
    assert bool((part[~inside] == 7.0).all())


def test_reference_on_inset_rects():
    """ref.jacobi5xk on a rect inset from its domain equals the same region
    of ref.jacobi5xk on the whole domain and writes nothing outside the rect
    (every rect and domain of A, B and D)."""
    geoms = _geoms()
    gen = torch.Generator(device="cpu").manual_seed(5)
    seen = set()
    cases = [tm.case_a(key, geoms[key[0], key[1]]) for key in tm.KEYS_A]
    cases += [tm.case_b(key, geoms[key[0], key[1]]) for key in tm.KEYS_B]
    for c in cases:
        sig = (c.k, c.mask, c.ncol, c.rect, c.dom)
        if sig in seen or c.rect == c.dom:  # (exact and scaled cases share shapes)
            continue
        seen.add(sig)
        h = torch.rand(c.dom[3] + 2 * c.k, c.ncol, generator=gen, dtype=torch.float64)
        _assert_rect_of(_ref(c.k, h, [c.rect], c.dom, c.mask), _ref(c.k, h, [c.dom], c.dom, c.mask), [c.rect])
    assert len(seen) >= 6 * (2 * 6 + 2)
    for k in tm.KS:
        for mask in tm.MASKS_D:
            for dw in tm.DW_D:
                nx, ny, xo = tm.nx_d(k, dw, geoms[k, 4]), tm.NY_D, 24 + dw % 2
                dom = (xo, nx, k, ny)
                h = torch.rand(ny + 2 * k, xo + nx + k + 3, generator=gen, dtype=torch.float64)
                core, frame = _engine_frame(k, xo, nx, k, ny, mask)
                assert core[1] >= geoms[k, 4]["GOUT"]
                whole = _ref(k, h, [dom], dom, mask)
                _assert_rect_of(_ref(k, h, [core], dom, mask), whole, [core])
                _assert_rect_of(_ref(k, h, frame, dom, mask), whole, frame)
