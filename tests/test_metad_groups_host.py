"""Metadynamics on CVs of groups of atoms without a GPU: the numpy model of a grouped bias against central
differences of its own energy, the closed forms of the coordination switch, the host build of cv_math.h (walked as the kernels
walk it) against the model, single-atom groups against the CVs of §18, the deposit chain against the analytic sum of Gaussians,
and what is refused at both levels.

Bars.  Finite differences: 10 |FD(h) - FD(h/2)| + 4 eps64 S_E / h at h = 1e-5 (§22's form): the first term is ten times the
change of the truncation error, the second the rounding of the two energies of a difference, each of which carries at most
eps64 S_E; S_E, the sum of the absolute addends of the energy, is the interpolant's (tests/_metad.py) plus |dV/ds_c| times the
absolute addends of s_c (sum|f| of a coordination CV, |s| of a CV of centres).  Header against model: `_metad_groups.cv_bars`
for the CVs, (gradient_depth + 1) / 2 + 2 half-ulp pairs for a force component (the lane's chunk, its splits, one more for an
atom of both sets, the exact model sum, then the product with dV and the sum over the CVs)."""

import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import _metad as M
import _metad_groups as G
from test_metad_host import _rocm_include, _torsion_atoms
from torchmd_amd.metadynamics import (GROUP_KINDS, Metadynamics, coord_phi, coord_switch, coordination_pairs, cv_dihedral, cv_distance,
                                      cv_of_centres)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "torchmd_amd", "csrc")
EPS64 = np.finfo(np.float64).eps
L = 20.0
KW = dict(height=1.0, frequency=1, temperature=300.0, bias_factor=6.0)


# ----------------------------------------------------------------------------- the cases
def _cloud(seed=2, N=90, box=L):
    rng = np.random.default_rng(seed)
    return rng.uniform(0.0, box if box else L, (N, 3)), np.where(rng.random(N) < 0.5, 1.008, 15.999)


def _filled(md, pos, box, offsets):
    """Five hills beside the CVs of `pos`: centres at s + off (per CV), heights 3, 2, 2.5, 1.5, 4."""
    s = md.cv_values(pos, np.asarray(box, dtype=np.float64))[0]
    grid = np.zeros_like(md.grid)
    for off, w in zip(offsets, (3.0, 2.0, 2.5, 1.5, 4.0)):
        grid += md.gauss_terms(s + np.asarray(off, dtype=np.float64)[: md.ncv], w)[None]
    return grid


OFF1 = [[0.25], [-0.4], [0.7], [1.9], [-2.2]]
OFF2 = [[0.5, 0.4], [-0.6, 0.5], [0.3, -0.7], [-0.4, -0.3], [1.0, 0.9]]


def _angle_atoms(theta, arm=2.0, origin=(6.0, 7.0, 8.0)):
    o = np.asarray(origin)
    return np.array([o + [arm, 0.0, 0.0], o, o + [1.5 * arm * np.cos(theta), 1.5 * arm * np.sin(theta), 0.0]])


def _case(name):
    """(Metadynamics, pos [N,3], box [3], grid) of the issue's cases."""
    pos, mass = _cloud()
    box = np.full(3, L)
    near = lambda c, n, skip=(), b=box: G.nearest(pos, c, n, b, skip)  # noqa: E731
    if name == "groups of 1, 2 and 40 atoms":
        md = Metadynamics([("group_angle", (near([5, 5, 5], 1), near([10, 10, 10], 40), near([15, 6, 12], 2))),
                           ("group_distance", (near([10, 10, 10], 40), near([4, 15, 15], 2)))], sigma=[0.2, 0.5], grid_min=[0.0, 1.0],
                          grid_max=[np.pi, 17.0], grid_bins=[40, 64], **KW)
        off = OFF2
    elif name == "a group wrapped across two faces":
        grp = near([0.2, 19.9, 10.0], 12)  # (around an edge of the box: its atoms lie on both sides of two faces)
        assert np.ptp(pos[grp][:, 0]) > 10.0 and np.ptp(pos[grp][:, 1]) > 10.0
        md = Metadynamics(("group_distance", (grp, near([6.0, 14.0, 11.0], 5, skip=grp))), sigma=0.5, grid_min=1.0, grid_max=17.0,
                          grid_bins=64, **KW)
        off = OFF1
    elif name == "the zero box":
        box = np.zeros(3)
        md = Metadynamics([("group_distance", (near([5, 5, 5], 6, b=box), near([12, 12, 12], 9, b=box))),
                           ("coordination", (near([8, 8, 8], 3, b=box), near([9, 9, 9], 30, b=box)), {"r0": 3.0, "n": 6})],
                          sigma=[0.5, 0.5], grid_min=[1.0, 0.0], grid_max=[25.0, 30.0], grid_bins=[96, 120], **KW)
        off = OFF2
    elif name == "one open axis":
        box = np.array([L, 0.0, L])
        pos[:, 1] -= 14.0
        md = Metadynamics([("group_distance", (near([0.5, -8, 19.5], 8, b=box), near([19.0, -6, 3.0], 8, b=box))),
                           ("coordination", (near([1.0, -4, 10], 2, b=box), near([19.5, -4, 10], 25, b=box)), {"r0": 3.0, "n": 6, "d_max": 8.0})],
                          sigma=[0.5, 0.4], grid_min=[1.0, 0.0], grid_max=[17.0, 20.0], grid_bins=[64, 100], **KW)
        off = OFF2
    elif name == "an atom in two groups and in both CVs":
        a = near([10, 10, 10], 10)
        b = a[:4] + near([14, 10, 10], 5, skip=a)
        md = Metadynamics([("group_distance", (a, b)), ("group_angle", (b, near([4, 4, 4], 3), {"atoms": a[2:8], "weights": [1, 2, 3, 4, 5, 6]}))],
                          sigma=[0.3, 0.2], grid_min=[0.0, 0.0], grid_max=[12.0, np.pi], grid_bins=[80, 40], **KW)
        off = [[0.2, 0.1], [-0.3, 0.3], [0.3, -0.3], [-0.2, -0.2], [0.5, 0.4]]
    elif name in ("a group dihedral just below +pi", "a group dihedral just above -pi"):
        phi = np.pi - 0.04 if "below" in name else -np.pi + 0.04
        x = _torsion_atoms(phi)
        pos = np.concatenate([x + [0.4, 0.0, 0.0], x - [0.4, 0.0, 0.0], pos[:4]])  # every centre the midpoint of two atoms
        mass = np.ones(len(pos))
        md = Metadynamics(("group_dihedral", ([0, 4], [1, 5], [2, 6], [3, 7])), sigma=0.35, grid_bins=48, **KW)
        md.masses = mass
        assert abs(md.cv_values(pos, box)[0][0] - phi) < 1e-9
        grid = np.zeros_like(md.grid)
        for s0, w in zip([np.pi - 0.5, -np.pi + 0.9, 2.4, -2.2, 1.7], [5.0, 1.0, 3.0, 0.5, 1.0]):
            grid += md.gauss_terms(np.array([s0]), w)[None]
        return md, pos, box, grid
    elif name in ("a group angle near 0", "a group angle near pi"):
        theta = 0.03 if "0" in name else np.pi - 0.03
        x = _angle_atoms(theta)
        pos = np.concatenate([x + [0.0, 0.0, 0.5], x - [0.0, 0.0, 0.5], pos[:3]])
        mass = np.ones(len(pos))
        md = Metadynamics(("group_angle", ([0, 3], [1, 4], [2, 5])), sigma=0.1, grid_min=0.0, grid_max=np.pi, grid_bins=80, **KW)
        md.masses = mass
        assert abs(md.cv_values(pos, box)[0][0] - theta) < 1e-9
        grid = np.zeros_like(md.grid)
        for s0, w in zip([0.1, 0.25, np.pi - 0.12, np.pi - 0.3, 1.5], [3.0, 2.0, 2.5, 1.5, 4.0]):
            grid += md.gauss_terms(np.array([s0]), w)[None]
        return md, pos, box, grid
    elif name == "s outside the grid":
        md = Metadynamics(("group_distance", (near([3, 3, 3], 4), near([12, 12, 12], 4))), sigma=0.5, grid_min=1.0, grid_max=9.0,
                          grid_bins=32, **KW)
        md.masses = mass
        s = md.cv_values(pos, box)[0][0]
        assert s > 9.5
        grid = np.zeros_like(md.grid)
        for s0, w in zip([s - 0.3, s + 0.2, 8.0, 8.8, 9.4], (3.0, 2.0, 2.5, 1.5, 4.0)):
            grid += md.gauss_terms(np.array([s0]), w)[None]
        return md, pos, box, grid
    elif name == "2-D, 24 x 20 bins":
        md = Metadynamics([("group_dihedral", (near([4, 4, 4], 3), near([7, 5, 4], 2), near([8, 8, 5], 3), near([11, 9, 8], 2))),
                           ("coordination", (near([10, 10, 10], 4), near([10, 10, 10], 40)), {"r0": 3.0, "n": 6, "d_max": 8.0})],
                          sigma=[0.55, 2.4], grid_min=[None, 0.0], grid_max=[None, 24.0], grid_bins=[24, 20], **KW)
        off = [[0.5, 1.6], [-0.6, 2.0], [0.3, -2.8], [-0.4, -1.2], [1.0, 3.6]]
    elif name == "coordination of one atom":
        # partners on both sides of d0 + r0 = 3.5 and of d_max = 8 (30 atoms within about 7.6 Å of the ion, 60 beyond)
        md = Metadynamics(("coordination", (near([10, 10, 10], 1), list(range(90))), {"r0": 3.0, "n": 6, "d0": 0.5, "d_max": 8.0}), sigma=0.4,
                          grid_min=0.0, grid_max=20.0, grid_bins=100, **KW)
        off = OFF1
    elif name == "coordination of overlapping sets":
        a = near([10, 10, 10], 12)
        md = Metadynamics(("coordination", (a, a[6:] + near([13, 10, 10], 14, skip=a)), {"r0": 3.0, "n": 8, "d_max": 8.0}), sigma=1.0,
                          grid_min=0.0, grid_max=200.0, grid_bins=400, **KW)
        off = [[0.6], [-1.0], [1.7], [4.0], [-5.0]]
    elif name == "coordination of a set with itself":
        a = near([10, 10, 10], 25)
        md = Metadynamics(("coordination", (a, a), {"r0": 3.0, "n": 6, "d_max": 8.0}), sigma=1.0, grid_min=0.0, grid_max=400.0, grid_bins=800, **KW)
        off = [[0.6], [-1.0], [1.7], [4.0], [-5.0]]
    else:
        raise KeyError(name)
    md.masses = mass
    return md, pos, box, _filled(md, pos, box, off)


CASES = ["groups of 1, 2 and 40 atoms", "a group wrapped across two faces", "the zero box", "one open axis",
         "an atom in two groups and in both CVs", "a group dihedral just below +pi", "a group dihedral just above -pi", "a group angle near 0",
         "a group angle near pi", "s outside the grid", "2-D, 24 x 20 bins", "coordination of one atom", "coordination of overlapping sets",
         "coordination of a set with itself"]


def _energy_addends(md, grid, pos, box):
    s, _ = md.cv_values(pos, box)
    dV = md.interp(grid[0], s)[1]
    S = M.interp_magnitude(md, grid[0], s)[0]
    for c in range(md.ncv):
        S += abs(dV[c]) * (G.coordination_magnitudes(md, c, pos, box)[0] if md.cv_kind[c] == 5 else abs(s[c]))
    return S


# ----------------------------------------------------------------------------- 1. the model against differences of its energy
@pytest.mark.parametrize("name", CASES)
def test_model_forces_are_minus_the_gradient_of_its_energy(name):
    md, pos, box, grid = _case(name)
    assert md.check_extent(pos, box)
    E, F, S = md.energy_forces(pos, box, grid)
    rows = md.row_atom
    probe = rows if len(rows) <= 14 else rows[np.linspace(0, len(rows) - 1, 14).astype(int)]
    energy = lambda x: md.energy_forces(x, box, grid)[0][0]  # noqa: E731
    h, S_E, worst = 1e-5, _energy_addends(md, grid, pos, box), 0.0
    untouched = np.ones(len(pos), dtype=bool)
    untouched[rows] = False
    assert np.all(F[0, untouched] == 0.0)
    if name == "s outside the grid":
        assert E[0] > 0.1 and np.all(F == 0.0)  # clamped: V constant (the tail of the hills), the force exactly zero
        for a in probe:
            x = pos.copy()
            x[a, 0] += h
            assert energy(x) == E[0]
        return
    assert E[0] > 0.1 and np.abs(F).max() > 0.05, (E, np.abs(F).max())
    for a in probe:
        for k in range(3):
            fd = []
            for hh in (h, 0.5 * h):
                xp, xm = pos.copy(), pos.copy()
                xp[a, k] += hh
                xm[a, k] -= hh
                fd.append(-(energy(xp) - energy(xm)) / (2.0 * hh))
            bar = 10.0 * abs(fd[0] - fd[1]) + 4.0 * EPS64 * S_E / h
            worst = max(worst, abs(F[0, a, k] - fd[1]) / bar)
            assert abs(F[0, a, k] - fd[1]) <= bar, (name, a, k, F[0, a, k], fd, bar)
    print(f"{name}: s = {S[0]}, V = {E[0]:.6f}, max|F| = {np.abs(F).max():.4f}, worst |F - FD| = {worst:.3f} of the bar")
    got = F[0, rows]
    assert np.abs(got.sum(axis=0)).max() <= 64 * EPS64 * np.abs(got).sum()  # functions of differences: no net force


def test_singular_angles_have_no_force():
    """theta = 0 and pi exactly (collinear centres) and a zero arm: the energy of the formula, the force exactly zero."""
    for x in (np.array([[2.0, 0, 0], [0, 0, 0], [3.0, 0, 0]]), np.array([[2.0, 0, 0], [0, 0, 0], [-3.0, 0, 0]]),
              np.array([[0.0, 0, 0], [0, 0, 0], [3.0, 0, 0]])):
        s, g = cv_of_centres(GROUP_KINDS["group_angle"], x + 5.0, np.full(3, L))
        assert s in (0.0, np.pi) and np.all(g == 0.0)
    md, pos, box, grid = _case("a group angle near 0")
    flat = pos.copy()
    flat[[2, 5]] = flat[[0, 3]] + [1.0, 0.0, 0.0]  # the third centre on the first arm
    E, F, S = md.energy_forces(flat, box, grid)
    assert S[0, 0] == 0.0 and E[0] > 0.1 and np.all(F == 0.0)


def test_transposed_grid_index_would_fail():
    md, pos, box, grid = _case("2-D, 24 x 20 bins")
    assert grid.shape == (1, 24, 21, 4)
    E = md.energy_forces(pos, box, grid)[0][0]
    wrong = grid.reshape(1, -1, 4).reshape(1, 21, 24, 4).transpose(0, 2, 1, 3)
    assert abs(md.energy_forces(pos, box, np.ascontiguousarray(wrong))[0][0] - E) > 1e-3 * abs(E)


# ----------------------------------------------------------------------------- 2. closed forms of the switch
def test_switch_closed_forms():
    r0, d0, d_max = 3.0, 0.5, 8.0
    for n in (2, 6, 7, 24):
        assert coord_phi(1.0, n)[0] == 0.5 and coord_switch(d0 + r0, r0, n, d0)[0] == 0.5  # r = d0 + r0: phi = 1/2 exactly
        assert coord_phi(1.0, n)[1] == -n / 4.0
        for x in (0.0, -0.0, -1.0, -1e300):
            assert coord_phi(x, n) == (1.0, 0.0)
        for r in (0.0, 0.25, d0):
            assert coord_switch(r, r0, n, d0) == (1.0, 0.0) and coord_switch(r, r0, n, d0, d_max) == (1.0, 0.0)
        # r = d_max and one ulp above: exactly 0 with zero slope; one ulp below: a few eps
        for r in (d_max, np.nextafter(d_max, np.inf), 2 * d_max, np.inf):
            assert coord_switch(r, r0, n, d0, d_max) == (0.0, 0.0)
        # One ulp below d_max: x differs from x_max by at most 2 ulp(x) (the subtraction is exact, the division rounds on both
        # sides), phi by |phi'| x that plus its own roundings: q (n - 1 half-ulps), q x, 1 + q x, 1 / den: (n + 2) / 2 eps phi
        # on either side; |phi' x| = n phi (1 - phi) <= n phi.  So |phi - phi_max| <= (2 n + n + 2) eps64 phi_max and
        # f <= (3 n + 2) eps64 phi_max / (1 - phi_max): at most 74 eps64 relative to phi_max for n = 24.
        below = float(np.nextafter(d_max, 0.0))
        f, df = coord_switch(below, r0, n, d0, d_max)
        phimax = float(coord_phi((d_max - d0) / r0, n)[0])
        count = 3 * n + 2
        assert 0.0 <= f <= count * EPS64 * phimax / (1.0 - phimax), (n, f, count)
        assert df < 0.0
        # monotone, and continuous through d_max
        rr = np.linspace(d0, d_max, 4001)
        ff = coord_switch(rr, r0, n, d0, d_max)[0]
        assert np.all(np.diff(ff) <= 0.0) and ff[0] == 1.0 and ff[-1] == 0.0
    # the rational switch (1 - x^n) / (1 - x^2n) away from its removable singularity
    x = np.array([0.3, 0.9, 1.1, 2.5])
    assert np.allclose(coord_phi(x, 6)[0], (1 - x**6) / (1 - x**12), rtol=1e-14)
    # the analytic slope against a difference
    for r in (1.0, 3.4, 3.6, 7.9):
        f1, f0 = coord_switch(r + 1e-6, r0, 6, d0, d_max)[0], coord_switch(r - 1e-6, r0, 6, d0, d_max)[0]
        assert abs((f1 - f0) / 2e-6 - coord_switch(r, r0, 6, d0, d_max)[1]) < 1e-8


def test_a_set_with_itself_counts_every_pair_twice_and_skips_i_equal_j():
    pos = np.array([[0.0, 0.0, 0.0], [3.0, 0.0, 0.0], [0.0, 4.0, 0.0], [9.0, 9.0, 9.0]])
    box, par = np.zeros(3), {"r0": 3.0, "n": 6}
    f = lambda r: float(coord_switch(r, 3.0, 6)[0])  # noqa: E731
    md = Metadynamics(("coordination", ([0, 1, 2], [0, 1, 2]), par), sigma=0.5, grid_min=0.0, grid_max=8.0, grid_bins=32, **KW)
    s = md.cv_values(pos, box)[0][0]
    assert abs(s - 2.0 * (f(3.0) + f(4.0) + f(5.0))) <= 4 * EPS64 * s and f(3.0) == 0.5
    one = Metadynamics(("coordination", ([0], [0]), par), sigma=0.5, grid_min=0.0, grid_max=8.0, grid_bins=32, **KW)
    assert one.cv_values(pos, box)[0][0] == 0.0  # i = j alone: nothing (not f(0) = 1)
    ab = Metadynamics(("coordination", ([0], [0, 1, 2]), par), sigma=0.5, grid_min=0.0, grid_max=8.0, grid_bins=32, **KW)
    assert abs(ab.cv_values(pos, box)[0][0] - (f(3.0) + f(4.0))) <= 4 * EPS64
    fm, gd = coordination_pairs(pos, box, [0, 1, 2], [0, 1, 2], **par)
    assert np.all(np.diag(fm) == 0.0) and np.array_equal(fm, fm.T) and np.array_equal(gd, -gd.transpose(1, 0, 2))


# ----------------------------------------------------------------------------- 3. the compiled header against the model
@pytest.fixture(scope="module")
def mg(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler (CXX, g++, c++, clang++) found: cv_math.h is not checked on the CPU")
    inc = _rocm_include()
    if inc is None:
        pytest.skip("the HIP headers (hip/hip_runtime.h) of a ROCm installation were not found: cv_math.h is not checked on the CPU")
    out = str(tmp_path_factory.mktemp("cv_math") / "libcv_math_host.so")
    cmd = [cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-D__HIP_PLATFORM_AMD__", f"-I{inc}", f"-I{CSRC}",
           os.path.join(HERE, "metad_group_math_host.cpp"), "-o", out]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, " ".join(cmd) + "\n" + res.stdout + res.stderr
    lib = C.CDLL(out)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    defn = [C.c_int64, C.c_int64, ip, ip, C.c_int64, ip, ip, dp, ip, dp, dp, dp, ip, dp, dp, dp]
    lib.mg_validate.restype = C.c_int
    lib.mg_validate.argtypes = defn + [C.c_char_p, C.c_int]
    lib.mg_check_box.restype = C.c_int
    lib.mg_check_box.argtypes = [C.c_double, C.c_int, C.c_double, C.c_double, dp, C.c_char_p, C.c_int]
    lib.mg_switch.restype = None
    lib.mg_switch.argtypes = [C.c_double, C.c_int, C.c_double, C.c_double, C.c_double, dp]
    lib.mg_nsplit.restype = C.c_int
    lib.mg_nsplit.argtypes = [C.c_int64, C.c_int64]
    lib.mg_bias.restype = C.c_int
    lib.mg_bias.argtypes = defn + [dp, dp, dp, dp, ip, dp, C.c_int]
    return lib


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def _defn(natoms, d, keep):
    """The definition of a group descriptor as the host program takes it."""
    i32 = lambda v: np.ascontiguousarray(list(v), dtype=np.int32)  # noqa: E731
    f64 = lambda v: np.ascontiguousarray(list(v), dtype=np.float64)  # noqa: E731
    arr = [i32(d.kind), i32([g for row in d.groups for g in row]), keep[0], keep[1], keep[2], i32(d.bins), f64(d.grid_min), f64(d.grid_max),
           f64(d.sigma), i32(d.coord_n), f64(d.coord_r0), f64(d.coord_d0), f64(d.coord_dmax)]
    args = [natoms, d.ncv, _ip(arr[0]), _ip(arr[1]), d.ngroups, _ip(arr[2]), _ip(arr[3]), _dp(arr[4]), _ip(arr[5]), _dp(arr[6]), _dp(arr[7]),
            _dp(arr[8]), _ip(arr[9]), _dp(arr[10]), _dp(arr[11]), _dp(arr[12])]
    return arr, args


def _host_bias(mg, md, pos, box, grid):
    d, keep = md.group_descriptor()
    arr, args = _defn(len(pos), d, keep)
    out, atom, force = np.zeros(5), np.zeros(len(pos), dtype=np.int32), np.zeros((len(pos), 3))
    g, p, b = np.ascontiguousarray(grid[0]), np.ascontiguousarray(pos), np.ascontiguousarray(box, dtype=np.float64)
    n = mg.mg_bias(*args, _dp(g), _dp(p), _dp(b), _dp(out), _ip(atom), _dp(force), len(pos))
    assert n == len(md.row_atom) and np.array_equal(atom[:n], md.row_atom)
    return out, force[:n]


@pytest.mark.parametrize("name", CASES + ["lattice: " + k for k in G.KERNEL_CASES])
def test_header_equals_model(mg, name):
    if name.startswith("lattice: "):
        pos, box, mass, md = G.kernel_case(name[9:], R=1)
        pos = pos[0]
        grid = G.prefill(md, pos[None], box)
    else:
        md, pos, box, grid = _case(name)
    E, F, S = md.energy_forces(pos, box, grid)
    out, force = _host_bias(mg, md, pos, box, grid)
    bars = G.cv_bars(md, pos, box)
    ds = np.abs(out[1:1 + md.ncv] - S[0])
    assert (ds <= bars).all(), (name, ds, bars)
    # V and dV at the host's own CVs: the interpolant's arithmetic alone (§18's bar: 16 eps64 x the magnitude of the terms)
    V, dV = md.interp(grid[0], out[1:1 + md.ncv])
    mv, md_ = M.interp_magnitude(md, grid[0], out[1:1 + md.ncv])
    assert abs(out[0] - V) <= 16 * EPS64 * mv and (np.abs(out[3:3 + md.ncv] - dV) <= 16 * EPS64 * np.maximum(md_, 1e-300)).all()
    # the gradients: the host's forces against -sum_c dV_c ds_c/dx of the model, with the host's own dV
    _, grads = md.group_cv_values(pos, box)
    want, mag = np.zeros_like(pos), np.zeros_like(pos)
    worst_c = 2.0
    for c in range(md.ncv):
        want += -out[3 + c] * grads[c]
        if md.cv_kind[c] == 5:
            nA, nB = (len(md.group_atoms[g]) for g in md.cv_groups[c])
            worst_c = max(worst_c, 0.5 * (G.gradient_depth(nA, nB) + 1) + 2.0)
            mag += abs(out[3 + c]) * G.coordination_magnitudes(md, c, pos, box)[1]
        else:
            # the addends of an atom's ds_c/dx: w_a ds/dX_g of every group of the CV that holds it (the model's, per group)
            gC = cv_of_centres(md.cv_kind[c], md.centres(pos, box)[md.cv_groups[c]], box)[1]
            for role, g in enumerate(md.cv_groups[c]):
                np.add.at(mag, md.group_atoms[g], abs(out[3 + c]) * np.abs(md.weights(g)[:, None] * gC[role]))
    err = np.abs(force - want[md.row_atom])
    ratio = (err / np.maximum(mag[md.row_atom], 1e-300)).max() / EPS64
    print(f"{name}: CVs {(ds / bars).max():.3f} of their bars (|ds| = {ds}), gradients {ratio:.2f} eps64 x sum|addends| (c = {worst_c:.1f})")
    assert (err <= worst_c * EPS64 * mag[md.row_atom]).all(), (name, ratio, worst_c)


def test_header_switch_equals_model(mg):
    out = np.zeros(2)
    rng = np.random.default_rng(1)
    for n in (2, 6, 12, 24):
        for d_max in (0.0, 8.0):
            for r in list(rng.uniform(0.0, 10.0, 200)) + [0.0, 0.5, 3.5, 8.0, float(np.nextafter(8.0, 0.0)), float(np.nextafter(8.0, 9.0))]:
                mg.mg_switch(3.0, n, 0.5, d_max, r, _dp(out))
                f, df = coord_switch(r, 3.0, n, 0.5, d_max if d_max else None)
                assert out[0] == f and out[1] == df, (n, d_max, r, out, f, df)  # the four operations alone: the same bits
    for nlane, nstream in ((1, 1), (1, 1025), (1, 98304), (32768, 32768), (257, 1000), (100, 32768), (98304, 1)):
        assert mg.mg_nsplit(nlane, nstream) == G.nsplit(nlane, nstream)


# ----------------------------------------------------------------------------- 4. single-atom groups
def test_single_atom_groups_are_the_cvs_of_atoms():
    rng = np.random.default_rng(3)
    equal = True
    for box in (np.full(3, L), np.zeros(3), np.array([L, 0.0, L])):
        for _ in range(50):
            pos = rng.uniform(-5.0, 25.0, (6, 3))
            gd = Metadynamics(("group_distance", ([4], [1])), sigma=0.5, grid_min=0.0, grid_max=40.0, grid_bins=160, **KW)
            gt = Metadynamics(("group_dihedral", ([0], [1], [2], [3])), sigma=0.35, grid_bins=48, **KW)
            gd.masses = gt.masses = np.ones(6)
            for md, (s_ref, g_ref), at in ((gd, cv_distance(pos[[4, 1]], box), [4, 1]), (gt, cv_dihedral(pos[[0, 1, 2, 3]], box), [0, 1, 2, 3])):
                s, grads = md.group_cv_values(pos, box)
                assert abs(s[0] - s_ref) <= 4 * EPS64 * abs(s_ref)
                assert (np.abs(grads[0][at] - g_ref[: len(at)]) <= 4 * EPS64 * np.abs(g_ref[: len(at)]).max()).all()
                equal = equal and s[0] == s_ref and np.array_equal(grads[0][at], g_ref[: len(at)])
    print(f"single-atom groups against cv_distance / cv_dihedral: {'equal to the bit' if equal else 'within 4 eps64, not bit-equal'}")
    # the old kinds beside a new one are served as such groups
    mixed = Metadynamics([("dihedral", (0, 1, 2, 3)), ("coordination", ([4], [5, 0]), {"r0": 3.0, "n": 6})], sigma=[0.35, 0.1],
                         grid_min=[None, 0.0], grid_max=[None, 3.0], grid_bins=[48, 60], **KW)
    assert mixed.grouped and mixed.cv_kind == [4, 5] and [len(a) for a in mixed.group_atoms] == [1, 1, 1, 1, 1, 2]
    assert all(np.array_equal(w, [1.0]) for w in mixed.group_weights[:4])
    pos = rng.uniform(0.0, 8.0, (6, 3))
    assert mixed.cv_values(pos, np.zeros(3))[0][0] == cv_dihedral(pos[:4], np.zeros(3))[0]
    old = Metadynamics([("dihedral", (0, 1, 2, 3)), ("distance", (4, 5))], sigma=[0.35, 0.3], grid_min=[None, 0.5], grid_max=[None, 6.5],
                       grid_bins=[48, 40], **KW)
    assert not old.grouped and old.descriptor().kind[1] == 0  # a bias of old kinds alone goes the old way


# ----------------------------------------------------------------------------- 5. deposition
def test_deposit_chain_converges_to_the_gaussian_sum():
    pos, mass = _cloud(seed=9)
    box = np.full(3, L)
    a = G.nearest(pos, [10, 10, 10], 1, box)
    errs = []
    rng = np.random.default_rng(6)
    pts = None
    for level in range(3):
        md = Metadynamics([("coordination", (a, list(range(90))), {"r0": 3.0, "n": 6, "d_max": 8.0}),
                           ("group_distance", (G.nearest(pos, [5, 5, 5], 6, box), G.nearest(pos, [12, 9, 8], 7, box)))], sigma=[0.4, 0.5],
                          grid_min=[0.0, 4.0], grid_max=[16.0, 14.0], grid_bins=[80 * 2 ** level, 40 * 2 ** level], height=1.0, frequency=1,
                          temperature=300.0, bias_factor=6.0)
        md.masses = mass
        assert np.allclose(md.h[:2], md.sigma[:2] / 2 ** (level + 1), rtol=1e-12)
        grid, hills = md.grid, []
        for k in range(5):
            pk = np.mod(pos + np.random.default_rng(40 + k).uniform(-0.5, 0.5, pos.shape), L)
            grid, rows = md.deposit_model(pk[None], box, grid)
            hills.append(rows[0])
        hills = np.asarray(hills)
        if level == 0:
            first = hills
        assert np.allclose(hills[:, :2], first[:, :2], rtol=0, atol=1e-12) and hills[1:, 2].min() < 0.999  # (well-tempered)
        lo, hi = hills[:, :2].min(axis=0) - 1.0, hills[:, :2].max(axis=0) + 1.0
        if pts is None:
            pts = rng.uniform(lo, hi, (400, 2))
        ev = ed = sv = sd = 0.0
        for s in pts:
            V, dV = md.interp(grid[0], s)
            Va, dVa = M.gaussian_sum(md, hills, s)
            ev, ed = max(ev, abs(V - Va)), max(ed, np.abs(dV - dVa).max())
            sv, sd = max(sv, abs(Va)), max(sd, np.abs(dVa).max())
        errs.append((ev / sv, ed / sd))
    rv = [errs[k][0] / errs[k + 1][0] for k in range(2)]
    rd = [errs[k][1] / errs[k + 1][1] for k in range(2)]
    print(f"relative errors (value, derivative) at h = sigma/2, /4, /8: {errs}; ratios value {rv}, derivative {rd}")
    assert errs[0][0] < 1e-3 and errs[0][1] < 1e-2
    assert min(rv) >= 10.0 and min(rd) >= 6.0


def test_shared_walkers_add_their_hills_in_replica_order_from_the_old_grid():
    pos, box, mass, md = G.kernel_case("coordination 1x257, 65x64 overlapping", R=4, walkers="shared")
    assert md.grid.shape[0] == 1
    grid, _ = md.deposit_model(G.moved(pos, 0, box), box, md.grid)
    old = grid.copy()
    p1 = G.moved(pos, 1, box)
    new, rows = md.deposit_model(p1, box, grid)
    assert np.array_equal(grid, old)
    want = old[0].copy()
    for r in range(4):
        s, _ = md.cv_values(p1[r], box)
        V, _ = md.interp(old[0], s)  # every height from the OLD grid
        assert np.array_equal(rows[r, :2], s) and rows[r, 2] == md.height * np.exp(-V / md.kdt)
        want = want + md.gauss_terms(s, rows[r, 2])
    assert np.array_equal(new[0], want) and len(set(rows[:, 2])) == 4 and (rows[:, 2] < md.height).any()


# ----------------------------------------------------------------------------- 6. what is refused
def _validate(mg, natoms, d, keep):
    arr, args = _defn(natoms, d, keep)
    why = C.create_string_buffer(256)
    mg.mg_validate(*args, why, 256)
    return why.value.decode()


def test_library_refusals(mg):
    def fresh():
        md = Metadynamics([("group_distance", ([0, 1, 2], {"atoms": [3, 4], "weights": [1.0, 2.0]})),
                           ("coordination", ([5], [5, 6, 7, 8]), {"r0": 3.0, "n": 6, "d0": 0.5, "d_max": 8.0})], sigma=[0.3, 0.2],
                          grid_min=[0.5, 0.0], grid_max=[6.5, 4.0], grid_bins=[40, 40], **KW)
        md.masses = np.ones(10)
        return md.group_descriptor()

    d, keep = fresh()
    assert _validate(mg, 10, d, keep) == ""

    def bad(expect, change, natoms=10):
        d, keep = fresh()
        change(d, keep)
        why = _validate(mg, natoms, d, keep)
        assert expect in why, (expect, why)

    def set_(name, value, *index):
        def change(d, keep):
            if not index:
                setattr(d, name, value)
            elif len(index) == 2:
                getattr(d, name)[index[0]][index[1]] = value
            else:
                getattr(d, name)[index[0]] = value
        return change

    poke = lambda which, where, value: (lambda d, keep: keep[which].__setitem__(where, value))  # noqa: E731
    bad("bad size", lambda d, keep: None, natoms=0)
    bad("at least one CV", set_("ncv", 0))
    bad("more than 2 CVs", set_("ncv", 3))
    bad("CV 0: unknown kind", set_("kind", 0, 0))  # (a plain distance is tmdhip_set_metadynamics's)
    bad("CV 1: unknown kind", set_("kind", 6, 1))
    bad("at least one group", set_("ngroups", 0))
    bad("start at 0", poke(0, 0, 1))
    bad("must not decrease", poke(0, 2, 2))
    bad("group 1 is empty", poke(0, 2, 3))
    bad("group 0: atom index out of range", poke(1, 1, 10))
    bad("atom index out of range", poke(1, 4, -1))
    bad("group 0: atom 0 is repeated", poke(1, 2, 0))
    bad("group 3: atom 5 is repeated", poke(1, 9, 5))
    bad("weights must be finite and > 0", poke(2, 3, 0.0))
    bad("weights must be finite and > 0", poke(2, 4, np.inf))
    bad("weights must be finite and > 0", poke(2, 0, np.nan))
    bad("CV 0: wrong number of groups", set_("groups", -1, 0, 1))
    bad("CV 0: wrong number of groups", set_("groups", 2, 0, 2))
    bad("CV 1: group index out of range", set_("groups", 4, 1, 1))
    bad("CV 0: a group is named twice", set_("groups", 0, 0, 1))
    bad("r0 must be finite and positive", set_("coord_r0", 0.0, 1))
    bad("r0 must be finite and positive", set_("coord_r0", np.inf, 1))
    bad("n must be a whole number in [2, 24]", set_("coord_n", 1, 1))
    bad("n must be a whole number in [2, 24]", set_("coord_n", 25, 1))
    bad("d0 must be finite and >= 0", set_("coord_d0", -0.5, 1))
    bad("d_max must lie above d0", set_("coord_dmax", 0.5, 1))
    bad("d_max must lie above d0", set_("coord_dmax", np.nan, 1))
    bad("sigma must be finite and positive", set_("sigma", 0.0, 0))
    bad("CV 1: sigma", set_("sigma", np.nan, 1))
    bad("bins must be positive", set_("bins", 0, 1))
    bad("grid_min must lie below grid_max", set_("grid_min", 6.5, 0))
    bad("CV 1: grid_min", set_("grid_max", np.nan, 1))
    bad("must not exceed sigma / 2", set_("bins", 39, 0))
    # a coordination CV with the same group twice is allowed (A = B), and a kind's unused CV slot is not read
    d, keep = fresh()
    d.groups[1][0] = 3
    assert _validate(mg, 10, d, keep) == ""
    d.ncv = 1
    d.kind[1] = 99
    assert _validate(mg, 10, d, keep) == ""
    # |A| |B| >= 2^31: offsets alone say so (the member table is not reached: the first group fails on its first index)
    off = np.array([0, 46341, 2 * 46341], dtype=np.int32)
    atoms, w = np.arange(2 * 46341, dtype=np.int32), np.ones(2 * 46341)
    big = Metadynamics(("coordination", ([0], [1]), {"r0": 3.0, "n": 6}), sigma=0.5, grid_min=0.0, grid_max=8.0, grid_bins=32, **KW)
    d, _ = big.group_descriptor()
    d.ngroups = 2
    assert "|A| |B| must stay below 2^31" in _validate(mg, 2 * 46341, d, [off, atoms, w])
    # the box: what run_check refuses
    why = C.create_string_buffer(256)
    box = lambda *b: _dp(np.array(b, dtype=np.float64))  # noqa: E731
    assert mg.mg_check_box(3.0, 6, 0.0, 8.0, box(20.0, 17.0, 0.0), why, 256) == 0
    assert mg.mg_check_box(3.0, 6, 0.0, 0.0, box(0.0, 0.0, 0.0), why, 256) == 0
    mg.mg_check_box(3.0, 6, 0.0, 0.0, box(0.0, 30.0, 0.0), why, 256)
    assert "needs d_max" in why.value.decode()
    mg.mg_check_box(3.0, 6, 0.0, 8.0, box(20.0, 15.9, 0.0), why, 256)
    assert "half the shortest non-zero box edge" in why.value.decode()


def test_python_refusals():
    ok = dict(sigma=0.3, grid_min=0.5, grid_max=6.5, grid_bins=40, **KW)
    sw = {"r0": 3.0, "n": 6, "d_max": 8.0}
    Metadynamics(("group_distance", ([0, 1], [2])), **ok)
    for expect, cvs, change in [
        ("unknown CV kind", [("angle", (0, 1, 2)), ("group_distance", ([0], [1]))], {"sigma": [0.3, 0.3], "grid_bins": [40, 40]}),
        ("unknown CV kind", ("angle", (0, 1, 2)), {}),
        ("unknown CV kind", ("rmsd", ([0, 1],)), {}),
        ("more than 2", [("group_distance", ([0], [1]))] * 3, {}),
        ("needs 2 groups", ("group_distance", ([0, 1], [2], [3])), {}),
        ("needs 3 groups", ("group_angle", ([0, 1], [2])), {}),
        ("needs 4 groups", ("group_dihedral", ([0], [1], [2])), {}),
        ("empty group", ("group_distance", ([], [2])), {}),
        ("repeats an atom", ("group_distance", ([0, 1, 0], [2])), {}),
        ("non-negative", ("group_distance", ([0, -1], [2])), {}),
        ("non-negative", ("group_distance", ([0.5, 1.0], [2])), {}),
        ("weights", ("group_distance", ({"atoms": [0, 1], "weights": [1.0, 0.0]}, [2])), {}),
        ("weights", ("group_distance", ({"atoms": [0, 1], "weights": [1.0, np.nan]}, [2])), {}),
        ("weights", ("group_distance", ({"atoms": [0, 1], "weights": [1.0]}, [2])), {}),
        ("a group is", ("group_distance", ({"atoms": [0, 1], "mass": [1.0, 1.0]}, [2])), {}),
        ("named twice", ("group_distance", ([0, 1], [0, 1])), {}),
        ("named twice", ("group_angle", ([0, 1], [2], [0, 1])), {}),
        ("coordination CV takes", ("coordination", ([0], [1, 2])), {}),
        ("coordination CV takes", ("coordination", ([0], [1, 2]), {"n": 6}), {}),
        ("coordination CV takes", ("coordination", ([0], [1, 2]), {"r0": 3.0, "m": 12}), {}),
        ("r0", ("coordination", ([0], [1, 2]), {**sw, "r0": 0.0}), {}),
        ("n must", ("coordination", ([0], [1, 2]), {**sw, "n": 1}), {}),
        ("n must", ("coordination", ([0], [1, 2]), {**sw, "n": 25}), {}),
        ("n must", ("coordination", ([0], [1, 2]), {**sw, "n": 6.5}), {}),
        ("d0", ("coordination", ([0], [1, 2]), {**sw, "d0": -1.0}), {}),
        ("d_max", ("coordination", ([0], [1, 2]), {**sw, "d0": 8.0}), {}),
        ("grid_min < grid_max", ("coordination", ([0], [1, 2]), sw), {"grid_min": None}),
        ("grid_min < grid_max", ("group_angle", ([0], [1], [2])), {"grid_max": None}),
        ("sigma / 2", ("group_distance", ([0], [1])), {"grid_bins": 39}),
        ("needs 2", [("distance", (0, 1, 2)), ("group_distance", ([0], [1]))], {"sigma": [0.3, 0.3], "grid_bins": [40, 40]}),
    ]:
        with pytest.raises(ValueError, match=expect):
            Metadynamics(cvs, **{**ok, **change})
    md = Metadynamics([("group_dihedral", ([0, 1], [2], [3], [4, 5])), ("coordination", ([0], [6, 7]), {"r0": 3.0})], sigma=[0.35, 0.2],
                      grid_min=[None, 0.0], grid_max=[None, 2.0], height=1.0, frequency=10, temperature=300.0)
    assert md.periodic == [True, False] and md.bins[0] == 36 and md.coord[1] == {"r0": 3.0, "n": 6, "d0": 0.0, "d_max": None}
    with pytest.raises(ValueError, match="needs masses"):
        md.cv_values(np.zeros((8, 3)), np.zeros(3))
    md.check(8, np.ones(8))
    assert np.array_equal(md.masses, np.ones(8))
    with pytest.raises(ValueError, match="beyond"):
        md.check(7)
    with pytest.raises(ValueError, match="no mass"):
        md.check(8, np.array([1.0, 1.0, 1.0, 1.0, 1.0, 0.0, 1.0, 1.0]))

    class Sites:
        nsites = 1
        sites = np.array([6])

    with pytest.raises(ValueError, match="virtual site"):
        md.check(8, np.ones(8), Sites())
    with pytest.raises(ValueError, match="needs d_max"):
        md.check_box([20.0, 20.0, 20.0])
    md.check_box(np.zeros(3))
    far = Metadynamics(("coordination", ([0], [1, 2]), sw), **ok)
    far.check_box([16.0, 30.0, 0.0])
    with pytest.raises(ValueError, match="half the shortest"):
        far.check_box([[30.0, 30.0, 30.0], [30.0, 15.9, 0.0]], R=2)
    # today's refusals stay
    for what in ("vmap", "batch", "barostat", "exchange", "domain"):
        assert md.refusal(what)
    with pytest.raises(ValueError, match="replicas"):
        md.energy_forces(np.zeros((2, 8, 3)), np.zeros(3))
    # the extent of a centre group
    x = np.zeros((8, 3))
    x[1, 0] = 10.0
    assert md.check_extent(x, np.full(3, 30.0)) and not md.check_extent(x, np.full(3, 20.0)) and md.check_extent(x, np.zeros(3))


def test_config_forms(tmp_path):
    np.save(tmp_path / "oxygens.npy", np.arange(0, 30, 3))
    conf = {"cvs": [["group_distance", [[0, 1, 2], [9, 10, 11]]], ["coordination", [[3], str(tmp_path / "oxygens.npy")], {"r0": 3.5, "n": 6, "d_max": 9.0}]],
            "sigma": [0.4, 0.2], "height": 1.0, "frequency": 10, "temperature": 300, "bias_factor": 6, "grid_min": [0.5, 0.0],
            "grid_max": [12.5, 8.0], "grid_bins": [60, 80]}
    md = Metadynamics.from_config(conf, 2)
    assert md.grouped and md.kinds == ["group_distance", "coordination"] and md.nreplicas == 2
    assert np.array_equal(md.group_atoms[3], np.arange(0, 30, 3)) and md.coord[1]["d_max"] == 9.0
    old = Metadynamics.from_config({**conf, "cvs": [["distance", [0, 30]], ["distance", [3, 60]]]}, 2)
    assert not old.grouped
    with pytest.raises(ValueError, match="cvs is a list"):
        Metadynamics.from_config({**conf, "cvs": [["coordination", [[3], [4]]], ["distance", [0, 1]]]}, 2)


def test_public_surface():
    import re

    from torchmd_amd import _lib as Lb
    from torchmd_amd import forces

    assert forces.SIDE_TERMS[-1] == "group_restraints" and len(forces.SIDE_TERMS) == 5
    hdr = open(os.path.join(ROOT, "include", "tmdhip.h")).read()
    assert re.search(r"#define TMDHIP_ABI_VERSION 11\b", hdr) and Lb.ABI_VERSION == 11
    assert "int tmdhip_set_metadynamics_groups(tmdhip_ctx *ctx, const tmdhip_metad_group_desc *desc);" in hdr
    assert "tmdhip_set_metadynamics_groups" in Lb.SIGNATURES
    for field, _ in Lb.MetadGroupDesc._fields_:
        assert re.search(r"\b" + field + r"\b", hdr[hdr.index("typedef struct tmdhip_metad_group_desc"):hdr.index("} tmdhip_metad_group_desc;")])
    assert C.sizeof(Lb.MetadGroupDesc) == 6 * 4 + 2 * 4 + 8 * 4 + 2 * 4 + 2 * 4 + 6 * 16 + 3 * 8
    from torchmd_amd import _build

    assert "metad_group.hip" in _build.SOURCES and "cv_math.h" in _build.HEADERS
