"""Well-tempered metadynamics without a GPU: the numpy model (`Metadynamics.energy_forces`, `deposit_model`)
against central finite differences of its own energy, the host build of metad_math.h against the model, the Hermite interpolant
against the analytic sum of Gaussians it stands for, the closed form of the well-tempered heights, shared walkers, what is
refused, and the splitting that keeps the bias out of the step kernels, checked in double.

Bars.  Finite differences: h = 1e-5 on energies of order 10 with third derivatives of order w / sigma^3: truncation ~1e-9
relative, rounding eps64 E / h ~ 1e-10: 1e-6 relative to the largest force component of the case, as §17.  Host build against
model: the same IEEE operations (the model spells its dot and cross products and its atan2 out in the header's order, so the
CVs are the same bits), libm's exp against numpy's: 16 eps64 x the sum of the magnitudes of the terms added.  Interpolant: orders 4 (value) and 3 (derivative), so
a halving of h divides the errors by 16 and 8; the bars are 10 and 6.  Splitting: as tests/test_restraints_host.py."""

import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import _metad as M
import _restraints as RS
from torchmd_amd.integrator import BOLTZMAN
from torchmd_amd.metadynamics import Metadynamics, cv_dihedral

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "torchmd_amd", "csrc")
EPS64 = np.finfo(np.float64).eps
L = 20.0


def _rocm_include():
    from torchmd_amd import _build

    try:
        hipcc = _build._hipcc()
    except RuntimeError:
        return None
    for root in (os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "/opt/rocm"):
        if os.path.exists(os.path.join(root, "include", "hip", "hip_runtime.h")):
            return os.path.join(root, "include")
    return None


@pytest.fixture(scope="module")
def mm(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler (CXX, g++, c++, clang++) found: metad_math.h is not checked on the CPU")
    inc = _rocm_include()
    if inc is None:
        pytest.skip("the HIP headers (hip/hip_runtime.h) of a ROCm installation were not found: metad_math.h is not checked on the CPU")
    out = str(tmp_path_factory.mktemp("metad_math") / "libmetad_math_host.so")
    cmd = [cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-D__HIP_PLATFORM_AMD__", f"-I{inc}", f"-I{CSRC}",
           os.path.join(HERE, "metad_math_host.cpp"), "-o", out]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, " ".join(cmd) + "\n" + res.stdout + res.stderr
    lib = C.CDLL(out)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    defn = [C.c_int64, ip, ip, ip, dp, dp, dp]
    lib.mm_validate.restype = C.c_int
    lib.mm_validate.argtypes = [C.c_int64] + defn + [C.c_char_p, C.c_int]
    lib.mm_bias.restype = C.c_int
    lib.mm_bias.argtypes = defn + [dp, dp, dp, dp, ip, dp]
    lib.mm_deposit.restype = C.c_int
    lib.mm_deposit.argtypes = defn + [dp, dp, C.c_double]
    lib.mm_height.restype = C.c_double
    lib.mm_height.argtypes = [C.c_double, C.c_double, C.c_double, C.c_int]
    return lib


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def _defn(md):
    """The definition of `md` as the host program (and tmdhip_metad_desc) takes it; the arrays are kept alive by the caller."""
    kind = np.array([{"distance": 0, "dihedral": 1}[k] for k in md.kinds] + [0] * (2 - md.ncv), dtype=np.int32)
    keep = [kind, np.ascontiguousarray(md.atoms, dtype=np.int32), np.ascontiguousarray(md.bins, dtype=np.int32),
            np.ascontiguousarray(md.grid_min), np.ascontiguousarray(md.grid_max), np.ascontiguousarray(np.resize(md.sigma, 2))]
    return keep, [md.ncv, _ip(keep[0]), _ip(keep[1]), _ip(keep[2]), _dp(keep[3]), _dp(keep[4]), _dp(keep[5])]


def _filled(md, centres, heights):
    """`md.grid` of grid 0 with hills at `centres` [n, ncv] of `heights` [n] added (every grid the same)."""
    grid = np.zeros_like(md.grid)
    for s0, w in zip(np.asarray(centres, dtype=np.float64).reshape(len(heights), md.ncv), heights):
        grid += md.gauss_terms(s0, w)[None]
    return grid


def _torsion_atoms(phi, origin=(3.0, 4.0, 5.0)):
    """Four atoms with bonds of 1.5 Å, right bond angles and the torsion `phi` (this package's sign)."""
    o = np.asarray(origin, dtype=np.float64)
    x = np.array([[1.5, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 1.5, 0.0], [1.5 * np.cos(phi), 1.5, -1.5 * np.sin(phi)]]) + o
    got = cv_dihedral(x, np.zeros(3))[0]
    if abs(np.angle(np.exp(1j * (got - phi)))) > 1e-9:  # (the other handedness)
        x[3, 2] = 2 * o[2] - x[3, 2]
    return x


def _one_distance(a, b, **kw):
    md = Metadynamics(("distance", (0, 1)), sigma=0.3, height=1.0, frequency=1, temperature=300.0, bias_factor=6.0, grid_min=0.5,
                      grid_max=6.5, grid_bins=40, **kw)
    return md, np.asarray([[a, b]], dtype=np.float64)


def _case(name):
    """(Metadynamics, pos [1,N,3], box, grid) of the issue's edge cases."""
    if name == "a distance across a face":
        md, pos = _one_distance([0.3, 4.0, 19.6], [19.5, 5.0, 0.2])
        box = [L, L, L]
    elif name == "one open axis":
        md, pos = _one_distance([0.3, -14.0, 19.6], [19.5, -12.7, 0.2])
        box = [L, 0.0, L]
    elif name == "s exactly on a node":
        md, pos = _one_distance([3.0, 4.0, 5.0], [3.0, 4.0, 5.0 + (0.5 + 12 * 0.15)])
        box = [L, L, L]
    elif name == "s outside the grid":
        md, pos = _one_distance([3.0, 4.0, 5.0], [3.0, 4.0, 5.0 + 6.9])
        box = [L, L, L]
    elif name in ("a dihedral just below +pi", "a dihedral just above -pi"):
        phi = np.pi - 0.04 if "below" in name else -np.pi + 0.04
        md = Metadynamics(("dihedral", (0, 1, 2, 3)), sigma=0.35, height=1.0, frequency=1, temperature=300.0, grid_bins=48)
        pos, box = _torsion_atoms(phi)[None], [L, L, L]
        assert abs(md.cv_values(pos[0], np.asarray(box))[0][0] - phi) < 1e-9
        return md, pos, box, _filled(md, [[np.pi - 0.5], [-np.pi + 0.9], [2.4], [-2.2], [1.7]], [5.0, 1.0, 3.0, 0.5, 1.0])
    else:  # "2-D, 24 x 20 bins": a dihedral and a distance across a face
        md = Metadynamics([("dihedral", M.PHI), ("distance", M.PAIR)], sigma=[0.55, 0.6], height=1.0, frequency=1, temperature=300.0,
                          grid_min=[None, 0.5], grid_max=[None, 6.5], grid_bins=[24, 20])
        pos, box, _, _ = M.kernel_case(R=1, seed=4)
        s = md.cv_values(pos[0], box)[0]
        cen = s + np.array([[0.5, 0.4], [-0.6, 0.5], [0.3, -0.7], [-0.4, -0.3], [1.0, 0.9]])
        return md, pos, box, _filled(md, cen, [3.0, 2.0, 2.5, 1.5, 2.0])
    s = md.cv_values(pos[0], np.asarray(box, dtype=np.float64))[0][0]
    return md, pos, box, _filled(md, [[s + 0.25], [s - 0.4], [s + 0.7], [5.9], [7.2]], [3.0, 2.0, 2.5, 1.5, 4.0])


CASES = ["a distance across a face", "one open axis", "a dihedral just below +pi", "a dihedral just above -pi", "s exactly on a node",
         "s outside the grid", "2-D, 24 x 20 bins"]


# ----------------------------------------------------------------------------- the model
@pytest.mark.parametrize("name", CASES)
def test_model_forces_are_minus_the_gradient_of_its_energy(name):
    md, pos, box, grid = _case(name)
    E, F, S = md.energy_forces(pos, box, grid)
    h = 1e-5
    num = np.zeros((len(md.row_atom), 3))
    for t, a in enumerate(md.row_atom):
        for c in range(3):
            p, m = pos.copy(), pos.copy()
            p[0, a, c] += h
            m[0, a, c] -= h
            num[t, c] = -(md.energy_forces(p, box, grid)[0][0] - md.energy_forces(m, box, grid)[0][0]) / (2 * h)
    got = F[0, md.row_atom]
    scale = np.abs(got).max()
    print(f"{name}: s = {S[0]}, V = {E[0]:.6f}, max|F| = {scale:.4f}, |F - FD| = {np.abs(num - got).max():.2e}")
    untouched = np.ones(pos.shape[1], dtype=bool)
    untouched[md.row_atom] = False
    assert np.all(F[0, untouched] == 0.0)
    if name == "s outside the grid":
        assert S[0, 0] > md.grid_max[0] and E[0] > 0.1  # (the tail of the hill centred outside)
        assert np.all(F == 0.0) and np.all(num == 0.0)  # clamped: V constant, the force exactly zero
        return
    assert E[0] > 0.1 and scale > 0.5
    assert np.abs(num - got).max() <= 1e-6 * scale, (num, got)
    assert np.abs(got.sum(axis=0)).max() <= 16 * EPS64 * np.abs(got).sum()  # a function of differences: no net force
    if name == "s exactly on a node":
        k = 12
        assert S[0, 0] == md.lo[0] + k * md.h[0]
        assert E[0] == grid[0, k, 0]  # the interpolant is exact on the nodes: the node's own value, to the bit


def test_transposed_grid_index_would_fail():
    """24 x 20 is not square on purpose: the model reads node (k0, k1) at k0 * 20 + k1, as the kernel does."""
    md, pos, box, grid = _case("2-D, 24 x 20 bins")
    assert grid.shape == (1, 24, 21, 4)
    E = md.energy_forces(pos, box, grid)[0][0]
    flat = grid.reshape(1, -1, 4)
    wrong = flat.reshape(1, 21, 24, 4).transpose(0, 2, 1, 3)
    assert abs(md.energy_forces(pos, box, np.ascontiguousarray(wrong))[0][0] - E) > 1e-3 * abs(E)


def test_portable_atan2_against_numpy():
    """metad_math.h's atan2 (the four operations alone, the same bits on the device, the host and here) is within 2 ulp of
    numpy's over twelve decades of |y / x| and on the axes."""
    from torchmd_amd.metadynamics import atan2_portable

    rng = np.random.default_rng(0)
    worst = 0.0
    for _ in range(20000):
        y, x = rng.standard_normal(2) * 10.0 ** rng.uniform(-3, 3, 2)
        a, b = atan2_portable(y, x), np.arctan2(y, x)
        worst = max(worst, abs(a - b) / np.spacing(abs(b)))
    assert worst <= 2.0
    for y, x in [(0.0, 1.0), (0.0, -1.0), (1.0, 0.0), (-1.0, 0.0), (0.0, 0.0), (1.0, 1.0), (-1.0, -1.0), (1e-300, 1.0), (1.0, 1e-300)]:
        assert atan2_portable(y, x) == np.arctan2(y, x)
    assert np.isnan(atan2_portable(np.nan, 1.0)) and np.isnan(atan2_portable(1.0, np.inf))


def test_dihedral_sign_is_the_bonded_term_s():
    """The reference's torsion (torchmd forces.py, as bonded_math.h evaluates it): -atan2(sin, cos) from r12 = x0 - x1,
    r23 = x1 - x2, r34 = x2 - x3."""
    rng = np.random.default_rng(2)
    for _ in range(20):
        x = M.chain(rng, [0.0, 0.0, 0.0], 4)
        r12, r23, r34 = x[0] - x[1], x[1] - x[2], x[2] - x[3]
        A, B = np.cross(r12, r23), np.cross(r23, r34)
        Cc = np.cross(r23, A)
        u = B / np.linalg.norm(B)
        ref = -np.arctan2(np.dot(Cc, u) / np.linalg.norm(Cc), np.dot(A, u) / np.linalg.norm(A))
        assert abs(cv_dihedral(x, np.zeros(3))[0] - ref) < 1e-12


# ----------------------------------------------------------------------------- the compiled header
def _host_bias(mm, md, grid_r, pos_r, box):
    keep, args = _defn(md)
    out, ra, rf = np.zeros(5), np.zeros(8, np.int32), np.zeros((8, 3))
    g = np.ascontiguousarray(grid_r)
    n = mm.mm_bias(*args, _dp(g), _dp(np.ascontiguousarray(pos_r)), _dp(np.ascontiguousarray(box, dtype=np.float64)), _dp(out), _ip(ra), _dp(rf))
    return out, ra[:n], rf[:n]


def test_header_equals_model(mm):
    worst = 0.0
    cases = [_case(n) for n in CASES]
    for second in ("dihedral", "distance", None):
        pos, box, _, md = M.kernel_case(R=2, second=second)
        grid = md.grid
        for k in range(5):
            grid, _ = md.deposit_model(M.moved(pos, k), box, grid)
        for r in range(2):
            cases.append((md, M.moved(pos, 7)[r:r + 1], box, grid[r:r + 1]))
    for md, pos, box, grid in cases:
        box = np.asarray(box, dtype=np.float64)
        s, g = md.cv_values(pos[0], box)
        V, dV = md.interp(grid[0], s)
        mv, mdv = M.interp_magnitude(md, grid[0], s)
        out, ra, rf = _host_bias(mm, md, grid[0], pos[0], box)
        assert np.array_equal(ra, md.row_atom)
        assert np.array_equal(out[1:1 + md.ncv], s)  # (atan2 by the four operations alone: the same bits)
        assert abs(out[0] - V) <= 16 * EPS64 * mv, (out[0], V)
        for c in range(md.ncv):
            assert abs(out[3 + c] - dV[c]) <= 16 * EPS64 * mdv[c], (c, out[3 + c], dV[c])
        F = np.zeros((len(md.row_atom), 3))
        mag = np.zeros_like(F)
        for t in range(len(md.row_atom)):
            for c in range(md.ncv):
                if md.row_role[t, c] >= 0:
                    F[t] += -dV[c] * g[c, md.row_role[t, c]]
                    mag[t] += mdv[c] * np.abs(g[c, md.row_role[t, c]])
        assert (np.abs(rf - F) <= 16 * EPS64 * mag).all(), (rf, F)
        if mag.max() > 0:
            worst = max(worst, (np.abs(rf - F) / np.where(mag > 0, mag, 1.0)).max() / EPS64)
    print(f"largest deviation header - model of a force component: {worst:.2f} eps64 x sum|terms|")


@pytest.mark.parametrize("second", ["dihedral", "distance", None])
def test_header_deposit_equals_model(mm, second):
    pos, box, _, md = M.kernel_case(R=1, second=second)
    keep, args = _defn(md)
    grid_m, grid_h, mag = md.grid.copy(), np.ascontiguousarray(md.grid[0].copy()), np.zeros_like(md.grid[0])
    for k in range(5):
        new, rows = md.deposit_model(M.moved(pos, k), box, grid_m)
        out, _, _ = _host_bias(mm, md, grid_h, M.moved(pos, k)[0], box)
        w = mm.mm_height(md.height, out[0], md.kdt, 0)
        assert abs(w - rows[0, md.ncv]) <= 16 * EPS64 * rows[0, md.ncv] * max(1.0, out[0] / md.kdt)
        assert np.array_equal(out[1:1 + md.ncv], rows[0, : md.ncv])  # the same centre to the bit: a centre one ulp off would move
        s0 = np.ascontiguousarray(out[1:3])                          # a far node's term by |Delta| / sigma^2 ulps
        assert mm.mm_deposit(*args, _dp(grid_h), _dp(s0), w) == md.width
        mag += np.abs(md.gauss_terms(rows[0, : md.ncv], rows[0, md.ncv]))
        grid_m = new
    dev = np.abs(grid_h - grid_m[0])
    assert grid_m[0, ..., 0].max() > 1.0
    print(f"{second}: grid after five hills, header - model: {(dev / np.maximum(mag, 1e-300)).max() / EPS64:.2f} eps64 x sum|terms|")
    assert (dev <= 16 * EPS64 * mag).all()


# ----------------------------------------------------------------------------- the interpolant against what it stands for
def _convergence(two_d):
    rng = np.random.default_rng(6)
    errs, pts = [], None
    for level in range(3):
        if two_d:
            nb = 32 * 2 ** level
            md = Metadynamics([("dihedral", (0, 1, 2, 3)), ("distance", (4, 5))], sigma=[2 * (2 * np.pi / 32), 0.5], height=1.0,
                              frequency=1, temperature=300.0, grid_min=[None, 0.0], grid_max=[None, 6.0], grid_bins=[nb, 24 * 2 ** level])
            cen = np.array([[-2.9, 1.0], [3.0, 2.2], [0.4, 3.1], [1.1, 4.9], [-1.3, 0.4]])
            lo, hi = np.array([-np.pi, 0.0]), np.array([np.pi, 6.0])
        else:
            md = Metadynamics(("distance", (0, 1)), sigma=0.4, height=1.0, frequency=1, temperature=300.0, grid_min=0.0, grid_max=8.0,
                              grid_bins=40 * 2 ** level)
            cen = np.array([[1.0], [1.7], [3.9], [5.2], [7.7]])
            lo, hi = np.array([0.0]), np.array([8.0])
        assert np.allclose(md.h[: md.ncv], md.sigma[: md.ncv] / 2 ** (level + 1), rtol=1e-12)
        w = np.array([1.0, 2.5, 0.7, 1.8, 1.2])
        grid = _filled(md, cen, w)[0]
        hills = np.concatenate([cen, w[:, None]], axis=1)
        if pts is None:  # (the same points on every level)
            pts = rng.uniform(lo, hi, (600, md.ncv))
        ev = ed = sv = sd = 0.0
        for s in pts:
            V, dV = md.interp(grid, s)
            Va, dVa = M.gaussian_sum(md, hills, s)
            ev, ed = max(ev, abs(V - Va)), max(ed, np.abs(dV - dVa).max())
            sv, sd = max(sv, abs(Va)), max(sd, np.abs(dVa).max())
        errs.append((ev / sv, ed / sd))
    return errs


@pytest.mark.parametrize("two_d", [False, True], ids=["1-D", "2-D"])
def test_interpolant_converges_to_the_gaussian_sum(two_d):
    errs = _convergence(two_d)
    rv = [errs[k][0] / errs[k + 1][0] for k in range(2)]
    rd = [errs[k][1] / errs[k + 1][1] for k in range(2)]
    print(f"{'2-D' if two_d else '1-D'}: relative errors (value, derivative) at h = sigma/2, /4, /8: {errs}; ratios value {rv}, derivative {rd}")
    assert errs[0][0] < 1e-3 and errs[0][1] < 1e-2  # (h = sigma / 2: the figures of the issue's table, 2.8e-4 and 3.1e-3)
    assert min(rv) >= 10.0 and min(rd) >= 6.0


# ----------------------------------------------------------------------------- deposition
def test_well_tempered_heights_on_a_node_follow_the_closed_form():
    md = Metadynamics(("distance", (0, 1)), sigma=0.25, height=1.5, frequency=1, temperature=300.0, bias_factor=5.0, grid_min=1.0,
                      grid_max=5.0, grid_bins=32)
    assert md.h[0] == 0.125
    pos = np.array([[[0.0, 0.0, 0.0], [2.5, 0.0, 0.0]]])  # s0 = node 12 exactly: no interpolation error
    kdt = BOLTZMAN * 4.0 * 300.0
    assert md.kdt == kdt
    grid, w = md.grid, []
    for _ in range(3):
        grid, rows = md.deposit_model(pos, np.zeros(3), grid)
        assert rows[0, 0] == 2.5
        w.append(rows[0, 1])
    want = [1.5, 1.5 * np.exp(-1.5 / kdt), 1.5 * np.exp(-(1.5 + 1.5 * np.exp(-1.5 / kdt)) / kdt)]
    for got, exp in zip(w, want):
        assert abs(got - exp) <= 4 * EPS64 * exp, (got, exp)
    assert grid[0, 12, 0] == (w[0] + w[1]) + w[2] and grid[0, 12, 1] == 0.0
    # plain metadynamics: every hill has the height itself
    pl = Metadynamics(("distance", (0, 1)), sigma=0.25, height=1.5, frequency=1, temperature=300.0, grid_min=1.0, grid_max=5.0, grid_bins=32)
    g, rows = pl.deposit_model(pos, np.zeros(3))
    g, rows = pl.deposit_model(pos, np.zeros(3), g)
    assert rows[0, 1] == 1.5 and pl.kdt is None
    # a hill centred outside a non-periodic grid still adds its tail to the nodes inside
    far = np.array([[[0.0, 0.0, 0.0], [5.3, 0.0, 0.0]]])
    g2, rows = pl.deposit_model(far, np.zeros(3))
    assert abs(rows[0, 0] - 5.3) < 1e-15 and g2[0, -1, 0] > 0.5
    assert abs(g2[0, -1, 0] - 1.5 * np.exp(-(0.3 * 0.3) / (2 * 0.25 * 0.25))) < 1e-14


def test_shared_walkers_add_their_hills_in_replica_order_from_the_old_grid():
    pos, box, _, md = M.kernel_case(R=4, second="distance", walkers="shared")
    assert md.grid.shape == (1, 48, 41, 4)
    grid = md.grid
    grid, _ = md.deposit_model(M.moved(pos, 0), box, grid)  # (so that the old grid is not flat)
    old = grid.copy()
    new, rows = md.deposit_model(M.moved(pos, 1), box, grid)
    assert np.array_equal(grid, old)  # (the argument is not changed)
    want = old[0].copy()
    for r in range(4):
        s, _ = md.cv_values(M.moved(pos, 1)[r], box)
        V, _ = md.interp(old[0], s)  # every height from the OLD grid
        assert np.array_equal(rows[r, :2], s) and rows[r, 2] == md.height * np.exp(-V / md.kdt)
        want = want + md.gauss_terms(s, rows[r, 2])
    assert np.array_equal(new[0], want)
    assert len(set(rows[:, 2])) == 4 and (rows[:, 2] < md.height).any()
    # independent walkers: one grid each, each seeing its own hills only
    pos, box, _, ind = M.kernel_case(R=4, second="distance")
    g, rows = ind.deposit_model(pos, box)
    for r in range(4):
        assert np.array_equal(g[r], ind.gauss_terms(rows[r, :2], rows[r, 2]))


def test_free_energy_bias_and_restart(tmp_path):
    md, pos, box, grid = _case("a distance across a face")
    md.set_grid(grid)
    V = md.energy_forces(pos, box)[0][0]
    s = md.cv_values(pos[0], np.asarray(box, dtype=np.float64))[0]
    assert md.bias(s) == V and np.array_equal(md.bias(np.array([[s[0]], [s[0]]])), [V, V])
    assert np.array_equal(md.free_energy(), -(6.0 / 5.0) * grid[..., 0])
    md.save(str(tmp_path / "bias.npz"))
    other, _, _, _ = _case("a distance across a face")
    other.load(str(tmp_path / "bias.npz"))
    assert np.array_equal(other.grid, grid) and other.nhills == 0 and other.hills().shape == (0, 1, 2)
    wrong = Metadynamics(("distance", (0, 1)), sigma=0.3, height=1.0, frequency=1, temperature=300.0, grid_min=0.5, grid_max=6.5,
                         grid_bins=80)
    with pytest.raises(ValueError, match="another grid"):
        wrong.load(str(tmp_path / "bias.npz"))


# ----------------------------------------------------------------------------- what is refused
def _validate(mm, natoms, ncv, kind, atoms, bins, gmin, gmax, sigma):
    arr = [np.ascontiguousarray(kind, dtype=np.int32), np.ascontiguousarray(atoms, dtype=np.int32).reshape(-1),
           np.ascontiguousarray(bins, dtype=np.int32), np.ascontiguousarray(gmin, dtype=np.float64),
           np.ascontiguousarray(gmax, dtype=np.float64), np.ascontiguousarray(sigma, dtype=np.float64)]
    why = C.create_string_buffer(256)
    mm.mm_validate(natoms, ncv, _ip(arr[0]), _ip(arr[1]), _ip(arr[2]), _dp(arr[3]), _dp(arr[4]), _dp(arr[5]), why, 256)
    return why.value.decode()


def test_library_refusals(mm):
    ok = dict(natoms=10, ncv=2, kind=[1, 0], atoms=[[0, 1, 2, 3], [4, 9, -1, -1]], bins=[48, 40], gmin=[0.0, 0.5], gmax=[0.0, 6.5],
              sigma=[0.35, 0.3])
    assert _validate(mm, **ok) == ""
    assert _validate(mm, **{**ok, "ncv": 1}) == ""
    bad = {
        "bad size": {"natoms": 0},
        "at least one": {"ncv": 0},
        "more than 2 CVs": {"ncv": 3},
        "unknown kind": {"kind": [2, 0]},
        "out of range": {"atoms": [[0, 1, 2, 10], [4, 9, -1, -1]]},
        "index out of range": {"atoms": [[0, 1, 2, 3], [4, -1, -1, -1]]},
        "is repeated": {"atoms": [[0, 1, 2, 1], [4, 9, -1, -1]]},
        "atom 4 is repeated": {"atoms": [[0, 1, 2, 3], [4, 4, -1, -1]]},
        "sigma must be finite": {"sigma": [0.35, np.inf]},
        "sigma must be finite and positive": {"sigma": [0.0, 0.3]},
        "CV 1: sigma": {"sigma": [0.35, np.nan]},
        "bins must be positive": {"bins": [48, 0]},
        "grid_min must lie below grid_max": {"gmin": [0.0, 6.5]},
        "CV 1: grid_min": {"gmax": [0.0, np.nan]},
        "must not exceed sigma / 2": {"bins": [35, 40]},       # 2 pi / 35 = 0.1795 > 0.175
        "CV 1: the grid spacing": {"sigma": [0.35, 0.29]},      # 0.15 > 0.145
    }
    for expect, change in bad.items():
        why = _validate(mm, **{**ok, **change})
        assert expect in why, (expect, why)
    assert _validate(mm, **{**ok, "bins": [36, 40]}) == ""  # 2 pi / 36 = 0.1745 <= 0.175


def test_python_refusals():
    ok = dict(sigma=0.3, height=1.0, frequency=10, temperature=300.0, grid_min=0.5, grid_max=6.5, grid_bins=40)
    Metadynamics(("distance", (0, 1)), **ok)
    for expect, cvs, change in [
        ("more than 2", [("distance", (0, 1)), ("distance", (2, 3)), ("distance", (4, 5))], {}),
        ("unknown CV kind", ("angle", (0, 1, 2)), {}),
        ("needs 2", ("distance", (0, 1, 2)), {}),
        ("needs 4", ("dihedral", (0, 1, 2)), {}),
        ("non-negative", ("distance", (0, -1)), {}),
        ("repeats an atom", ("distance", (3, 3)), {}),
        ("repeats an atom", ("dihedral", (0, 1, 2, 0)), {}),
        ("sigma", ("distance", (0, 1)), {"sigma": 0.0}),
        ("sigma", ("distance", (0, 1)), {"sigma": np.nan}),
        ("height", ("distance", (0, 1)), {"height": -1.0}),
        ("height", ("distance", (0, 1)), {"height": np.inf}),
        ("frequency", ("distance", (0, 1)), {"frequency": 0}),
        ("frequency", ("distance", (0, 1)), {"frequency": 2.5}),
        ("temperature", ("distance", (0, 1)), {"temperature": 0.0}),
        ("bias_factor", ("distance", (0, 1)), {"bias_factor": 1.0}),
        ("grid_min < grid_max", ("distance", (0, 1)), {"grid_min": 6.5}),
        ("grid_min < grid_max", ("distance", (0, 1)), {"grid_min": None}),
        ("grid_bins", ("distance", (0, 1)), {"grid_bins": 0}),
        ("grid_bins", ("distance", (0, 1)), {"grid_bins": [40, 40]}),
        ("sigma / 2", ("distance", (0, 1)), {"grid_bins": 39}),
        ("nreplicas", ("distance", (0, 1)), {"nreplicas": 0}),
        ("walkers", ("distance", (0, 1)), {"walkers": "both"}),
    ]:
        with pytest.raises(ValueError, match=expect):
            Metadynamics(cvs, **{**ok, **change})
    md = Metadynamics(("dihedral", (0, 1, 2, 4)), sigma=0.35, height=1.0, frequency=10, temperature=300.0)  # bins chosen: h <= sigma / 2
    assert md.bins[0] == 36 and md.grid.shape == (1, 36, 2)
    md.check(5, np.ones(5))
    with pytest.raises(ValueError, match="beyond"):
        md.check(4)
    with pytest.raises(ValueError, match="no mass"):
        md.check(5, np.array([1.0, 1.0, 0.0, 1.0, 1.0]))

    class Sites:
        nsites = 1
        sites = np.array([4])

    with pytest.raises(ValueError, match="virtual site"):
        md.check(5, np.ones(5), Sites())
    with pytest.raises(ValueError, match="replicas"):
        md.energy_forces(np.zeros((2, 5, 3)), np.zeros(3))
    with pytest.raises(ValueError, match="the grid is"):
        md.set_grid(np.zeros((1, 35, 2)))


def test_public_surface_and_forces_keyword():
    import inspect

    import torchmd_amd
    from torchmd_amd.forces import Forces

    assert torchmd_amd.Metadynamics is Metadynamics and "Metadynamics" in torchmd_amd.__all__
    params = list(inspect.signature(Forces.__init__).parameters)
    assert "metadynamics" in params
    from torchmd_amd.domain import DomainSet

    md = Metadynamics(("dihedral", (0, 1, 2, 4)), sigma=0.35, height=1.0, frequency=10, temperature=300.0)
    with pytest.raises(ValueError, match="metadynamics"):
        DomainSet(np.full(3, 30.0), 2, "cpu", None, ["lj"], 9.0, dry=True, metadynamics=md)


# ----------------------------------------------------------------------------- the splitting
@pytest.mark.parametrize("gdt", [0.0, 0.05])
def test_impulse_scheme_equals_bias_inside_the_force(gdt):
    toy = M.BiasToy()
    dt = 0.02
    gamma = gdt / dt
    cuts = (1, 4, 7)
    steps = sum(cuts)
    xi, vi, fi, hills_i = M.run_cut_depositing(RS.run_inside, toy, cuts, dt, gamma)
    grid_i = toy.grid.copy()
    assert np.abs(xi - toy.x0).max() > 0.05 and len(hills_i) == 2  # (something happened; a deposition between the cuts)
    fb = np.abs(toy.f_restraint(toy.x0)).max()
    assert fb > 2.0  # (a bias force worth integrating)
    bar_x = 64 * EPS64 * steps * np.abs(xi).max()
    bar_v = 64 * EPS64 * steps * max(np.abs(vi).max(), np.abs(xi).max() / dt / steps)
    xs, vs, fs, hills_s = M.run_cut_depositing(RS.run_impulse, toy, cuts, dt, gamma)
    dx, dv = np.abs(xs - xi).max(), np.abs(vs - vi).max()
    print(f"gamma dt = {gdt}: |F_b| = {fb:.2f}, |dx| = {dx:.2e} (bar {bar_x:.2e}), |dv| = {dv:.2e} (bar {bar_v:.2e})")
    assert dx <= bar_x and dv <= bar_v
    assert np.abs(fs - fi).max() <= 64 * EPS64 * steps * np.abs(fi).max()  # the force buffer carries F_b across calls
    # the hills of the two schemes sit where the trajectories are, and weigh what the grids say
    for a, b in zip(hills_i, hills_s):
        assert np.abs(a - b).max() <= 64 * EPS64 * steps * np.abs(a).max()
    assert np.abs(toy.grid - grid_i).max() <= 1e-9 * np.abs(grid_i).max()
    assert hills_i[1][0, 1] < hills_i[0][0, 1] < toy.md.height  # well-tempered: on top of a bias the hills shrink
    # controls: dt/2 in place of dt, and (with friction) the compensation left out, miss the bar by more than 10^3
    xh = M.run_cut_depositing(RS.run_impulse, toy, cuts, dt, gamma, interior_kick=0.5 * dt / (1.0 - gamma * dt))[0]
    assert np.abs(xh - xi).max() > 1e3 * bar_x
    if gdt:
        xn = M.run_cut_depositing(RS.run_impulse, toy, cuts, dt, gamma, interior_kick=dt)[0]
        print(f"  compensation left out: |dx| = {np.abs(xn - xi).max():.2e}")
        assert np.abs(xn - xi).max() > 1e3 * bar_x
