"""The cell grid's planner (torchmd_amd/csrc/grid_plan.h: plan_grid_host, row_zreach, read_stencil_knob) compiled for the
host and checked against geometry worked out here from the cell edges — no GPU.

tests/grid_plan_host.cpp wraps the header behind a C interface; a module-scoped fixture compiles it with the system C++ compiler
and loads it with ctypes (the header needs no HIP).  Without a host compiler the module skips and says so.

What is checked, for a few hundred random orthorhombic and open boxes and every stencil half-width m in {1, 2, 3}:
  - a periodic axis never gets fewer than 2m + 1 cells (a stencil would meet a cell twice); otherwise the plan steps down to a
    smaller m or is refused;
  - zreach[ox][oy] is exactly the largest |oz| whose cell — an axis-aligned brick of the planned edges, (ox, oy, oz) cells
    away from the home cell — comes within rlist of the home cell, the distance between two bricks taken per axis from their
    corner coordinates; -1 only where no brick of the row does.  A smaller value would drop pairs, a larger one is wasted work;
  - cubic boxes plan what the library planned before the arithmetic moved into the header (PARENT, a table of twelve boxes
    printed by the previous plan_grid compiled as it stood)."""

import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "torchmd_amd", "csrc")
UNSET = 99  # what grid_plan_host.cpp fills zreach with before the planner runs


@pytest.fixture(scope="module")
def gp(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler (CXX, g++, c++, clang++) found: grid_plan.h is not checked on the CPU")
    out = str(tmp_path_factory.mktemp("grid_plan") / "libgrid_plan_host.so")
    cmd = [cxx, "-std=c++17", "-O2", "-fPIC", "-shared", f"-I{CSRC}", os.path.join(HERE, "grid_plan_host.cpp"), "-o", out]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, " ".join(cmd) + "\n" + res.stdout + res.stderr
    lib = C.CDLL(out)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    lib.gp_plan.argtypes = [C.c_int, C.c_double, dp, dp, dp, C.c_int, ip, ip, dp]
    return lib


def plan(gp, natoms, rlist, box, lo=(0, 0, 0), hi=(0, 0, 0), knob=0):
    """-> None (refused) or dict(m, nc, periodic, zreach [2m+1, 2m+1], rest (the 7 x 7 entries outside the stencil), inv_edge, origin)"""
    d3 = C.c_double * 3
    out, z, real = (C.c_int * 5)(), (C.c_int * 49)(), (C.c_double * 6)()
    if not gp.gp_plan(natoms, rlist, d3(*box), d3(*lo), d3(*hi), knob, out, z, real):
        return None
    m = out[3]
    z = np.array(list(z)).reshape(7, 7)
    inside = np.zeros((7, 7), dtype=bool)
    inside[: 2 * m + 1, : 2 * m + 1] = True
    return dict(m=m, nc=tuple(out[:3]), periodic=out[4], zreach=z[: 2 * m + 1, : 2 * m + 1], rest=z[~inside],
                inv_edge=np.array(real[:3]), origin=np.array(real[3:]))


def brick_distance2(offset, edge):
    """Squared distance between the home cell [0, e] per axis and the cell `offset` cells away, from the corner coordinates."""
    d2 = 0.0
    for o, e in zip(offset, edge):
        lo, hi = o * e, (o + 1) * e
        d2 += max(0.0, lo - e, 0.0 - hi) ** 2
    return d2


def expected_zreach(m, edge, rlist):
    """(zreach [2m+1, 2m+1], True where some brick sits within 1e-9 relative of rlist: a comparison not to be judged)"""
    z = -np.ones((2 * m + 1, 2 * m + 1), dtype=int)
    marginal = np.zeros_like(z, dtype=bool)
    for ox in range(-m, m + 1):
        for oy in range(-m, m + 1):
            for oz in range(0, m + 1):
                d2 = brick_distance2((ox, oy, oz), edge)
                assert abs(d2 - brick_distance2((ox, oy, -oz), edge)) <= 1e-12 * max(d2, 1.0)  # (a row's reach is symmetric in z)
                marginal[ox + m, oy + m] |= abs(d2 - rlist * rlist) <= 1e-9 * rlist * rlist
                if d2 <= rlist * rlist:
                    z[ox + m, oy + m] = oz
    return z, marginal


def check_plan(p, natoms, rlist, len3, periodic, knob):
    m, nc = p["m"], np.array(p["nc"])
    assert 1 <= m <= (knob if knob > 0 else 2)
    assert p["periodic"] == int(periodic)
    want = np.minimum(np.maximum(np.floor(len3 / (rlist / m)).astype(int), 1), 1024)
    assert (nc == want).all(), (nc, want)
    if periodic:
        assert (nc >= 2 * m + 1).all(), (nc, m)
    edge = len3 / nc
    assert np.allclose(p["inv_edge"], 1.0 / edge, rtol=1e-14)
    # m cells cover rlist (an axis of 1 024 cells has longer ones, an open axis shorter than one cell is one cell)
    assert (edge[(nc > 1) & (nc < 1024)] >= rlist / m * (1 - 1e-14)).all()
    z, marginal = expected_zreach(m, edge, rlist)
    ok = (p["zreach"] == z) | marginal
    assert ok.all(), (m, edge, rlist, p["zreach"], z)
    assert (z[m, m] == m) and (p["zreach"] >= -1).all() and (p["zreach"] <= m).all()
    assert (p["rest"] == UNSET).all()  # nothing written outside the stencil
    return (z < m).any(), (z < 0).any()


@pytest.mark.parametrize("knob", [1, 2, 3, 0])
def test_random_boxes_plan_complete_and_tight_stencils(gp, knob):
    rng = np.random.default_rng(100 + knob)
    trimmed = dropped = refused = stepped_down = 0
    for case in range(300):
        rlist = rng.uniform(6.0, 14.0)
        periodic = case % 3 != 0
        # edges from just under three coarse cells to a few tens of fine ones, independent per axis
        len3 = rlist * rng.uniform(0.9, 1.0, 3) * rng.choice([1.05, 2.7, 3.4, 3.6, 4.1, 5.2, 7.7, 9.3], 3)
        natoms = int(rng.choice([0.002, 0.02, 0.1]) * len3.prod()) + 1
        lo = rng.uniform(-50, 50, 3)
        p = plan(gp, natoms, rlist, len3 if periodic else (0, 0, 0), lo, lo + len3, knob)
        mmax = knob if knob > 0 else 2
        fits = [m for m in range(mmax, 0, -1) if not periodic or (np.floor(len3 / (rlist / m)) >= 2 * m + 1).all()]
        if p is None:
            # refused: only a periodic box that is too small for every half-width (m = 1 has no atoms-per-cell rule)
            assert periodic and 1 not in fits, (len3, rlist)
            refused += 1
            continue
        assert p["m"] in fits, (p["m"], fits, len3, rlist)
        assert np.allclose(p["origin"], 0.0 if periodic else lo)
        stepped_down += p["m"] < mmax
        t, d = check_plan(p, natoms, rlist, len3, periodic, knob)
        trimmed += t
        dropped += d
    # the draw reaches what the checks are about: trimmed rows (and, at m = 3, rows with no cell in reach), refusals, smaller m
    # (a smaller m than the largest one tried comes from the atoms-per-cell rules alone: a periodic box too small for m = 2 or 3
    # is too small for every smaller m as well, and the knob switches the rule of m = 2 off)
    assert refused >= 5 and (stepped_down >= 5 or knob in (1, 2)), (refused, stepped_down)
    if knob >= 2:
        assert trimmed >= 10, trimmed
    if knob == 3:
        assert dropped >= 1, dropped


def test_atoms_per_cell_rules(gp):
    rl = 10.2
    # m = 3 needs two atoms per cell
    box = (40.0, 44.0, 52.0)  # m = 3: 11 x 12 x 15 = 1 980 cells
    assert plan(gp, 3960, rl, box, knob=3)["m"] == 3 and plan(gp, 3960, rl, box, knob=3)["nc"] == (11, 12, 15)
    assert plan(gp, 3959, rl, box, knob=3)["m"] == 2
    # m = 2 below four atoms per cell steps down to m = 1 — where m = 1 fits, and only without the knob
    box = (41.0, 46.0, 62.0)  # m = 2: 8 x 9 x 12 = 864 cells; m = 1: 4 x 4 x 6
    assert plan(gp, 3456, rl, box)["m"] == 2
    p = plan(gp, 3455, rl, box)
    assert p["m"] == 1 and p["nc"] == (4, 4, 6)
    assert plan(gp, 3455, rl, box, knob=2)["m"] == 2
    assert plan(gp, 3455, rl, box, knob=-1)["m"] == 2  # (the variable set to something that is no half-width)
    assert plan(gp, 10, rl, (30.5, 46.0, 62.0))["m"] == 2  # 30.5 A: two coarse cells only, the sparse grid keeps m = 2
    # open boxes: no minimum cell count, one cell at the least, 1 024 at the most
    p = plan(gp, 3000, rl, (0, 0, 0), (-3.0, 0.0, 0.0), (10460.0, 52.0, 4.0))
    assert p["m"] == 1 and p["nc"] == (1024, 5, 1) and p["periodic"] == 0
    p = plan(gp, 400000, rl, (0, 0, 0), (0, 0, 0), (6000.0, 52.0, 52.0), knob=2)
    assert p["m"] == 2 and p["nc"] == (1024, 10, 10)
    assert plan(gp, 100, rl, (30.7, 0.0, 30.7)) is None  # a periodic box needs three positive edges


def test_stencil_knob_parsing(gp, monkeypatch):
    monkeypatch.delenv("TMDHIP_STENCIL", raising=False)
    assert gp.gp_read_stencil_knob() == 0
    for val, want in (("1", 1), ("2", 2), ("3", 3), ("0", -1), ("4", -1), ("x", -1), ("", -1)):
        monkeypatch.setenv("TMDHIP_STENCIL", val)
        assert gp.gp_read_stencil_knob() == want, val


# (box edge, atoms, rlist) -> (m, cells per axis, zreach) or None, from plan_grid before it called grid_plan.h
_FULL2, _FULL1 = [[2] * 5] * 5, [[1] * 3] * 3
PARENT = [
    ((37.264, 5184, 10.2), (2, (7, 7, 7), _FULL2)),
    ((49.686, 12288, 10.2), (2, (9, 9, 9), _FULL2)),
    ((99.365, 98304, 10.2), (2, (19, 19, 19), _FULL2)),
    ((30.7, 3000, 10.2), (2, (6, 6, 6), _FULL2)),
    ((30.5, 3000, 10.2), (2, (5, 5, 5), [[1, 2, 2, 2, 1], [2, 2, 2, 2, 2], [2, 2, 2, 2, 2], [2, 2, 2, 2, 2], [1, 2, 2, 2, 1]])),
    ((25.6, 1700, 10.2), (2, (5, 5, 5), _FULL2)),
    ((25.4, 1700, 10.2), None),
    ((72.16, 8000, 10.2), (1, (7, 7, 7), _FULL1)),
    ((360.8, 1000000, 9.7), (1, (37, 37, 37), _FULL1)),
    ((61.3, 900, 10.2), (1, (6, 6, 6), _FULL1)),
    ((41.0, 6900, 13.2), (2, (6, 6, 6), _FULL2)),
    ((20.0, 800, 10.2), None),
]


def test_cubic_boxes_plan_what_the_library_planned_before(gp):
    for (L, natoms, rlist), want in PARENT:
        p = plan(gp, natoms, rlist, (L, L, L))
        if want is None:
            assert p is None, (L, natoms, rlist)
            continue
        assert (p["m"], p["nc"], p["zreach"].tolist()) == want, (L, natoms, rlist)
