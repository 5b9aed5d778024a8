"""Shared pieces of the metadynamics tests: the random systems of the kernel tests (a peptide-like chain whose
phi / psi dihedrals share three atoms, a distance across a box face), the magnitude of the terms the interpolant sums, the
analytic sum of Gaussians the interpolant stands for, and the toy of tests/_restraints.py with a tabulated bias in the place of
its restraints (the splitting, on the host)."""

import numpy as np

import _restraints as RS
from torchmd_amd.metadynamics import Metadynamics, hermite_basis, locate

EPS64 = np.finfo(np.float64).eps

PHI, PSI = (10, 11, 12, 13), (11, 12, 13, 14)  # share three atoms: five distinct rows
PAIR = (21, 20)                                 # a distance across a face


def _unit(v):
    return v / np.linalg.norm(v)


def chain(rng, start, nat=5, bond=1.5, lo=65.0, hi=115.0):
    """`nat` atoms from `start` with bonds of `bond` Å, bond angles drawn from [lo, hi] degrees and torsions from [-pi, pi)."""
    pts = [np.asarray(start, dtype=np.float64)]
    pts.append(pts[0] + bond * _unit(rng.standard_normal(3)))
    fake = pts[0] + _unit(rng.standard_normal(3))
    for k in range(2, nat):
        a, b, c = (fake if k == 2 else pts[k - 3]), pts[k - 2], pts[k - 1]
        th, tau = np.radians(rng.uniform(lo, hi)), rng.uniform(-np.pi, np.pi)
        bc = _unit(c - b)
        n = _unit(np.cross(b - a, bc))
        d = np.array([-bond * np.cos(th), bond * np.sin(th) * np.cos(tau), bond * np.sin(th) * np.sin(tau)])
        pts.append(c + d[0] * bc + d[1] * np.cross(n, bc) + d[2] * n)
    return np.stack(pts)


def bond_angles(x):
    out = []
    for k in range(1, len(x) - 1):
        u, v = x[k - 1] - x[k], x[k + 1] - x[k]
        out.append(np.degrees(np.arccos(np.dot(u, v) / np.linalg.norm(u) / np.linalg.norm(v))))
    return np.asarray(out)


def kernel_case(R=3, N=200, seed=11, L=20.0, second="dihedral", walkers="independent", bias_factor=6.0):
    """R replicas of N random atoms in a cubic box of edge L, masses in {1.008, 15.999}.  Atoms 10..14 are a chain that starts
    within 1 Å of the box face x = L (wrapped back into the box, so some of its bonds cross the face); atoms 20, 21 sit on
    either side of the face y = 0.  CVs: phi = (10, 11, 12, 13) and psi = (11, 12, 13, 14) on a 48 x 40 grid, or, with
    second="distance", phi and the distance 21-20 (sigma 0.3 on [0.5, 6] in 40 bins).
    Returns (pos [R,N,3], box [3], mass [N], Metadynamics)."""
    rng = np.random.default_rng(seed)
    pos = rng.uniform(0.0, L, (R, N, 3))
    for r in range(R):
        c = chain(rng, [L - rng.uniform(0.1, 1.0), rng.uniform(5.0, 15.0), rng.uniform(5.0, 15.0)])
        pos[r, 10:15] = np.mod(c, L)
        pos[r, 20] = [rng.uniform(5, 15), L - rng.uniform(0.2, 1.2), rng.uniform(5, 15)]
        pos[r, 21] = pos[r, 20] + [rng.uniform(-0.8, 0.8), rng.uniform(1.5, 2.5), rng.uniform(-0.8, 0.8)]
        pos[r, 21] = np.mod(pos[r, 21], L)
    mass = np.where(rng.random(N) < 0.6, 1.008, 15.999)
    if second == "dihedral":
        md = Metadynamics([("dihedral", PHI), ("dihedral", PSI)], sigma=[0.35, 0.4], height=1.2, frequency=1, temperature=300.0,
                          bias_factor=bias_factor, grid_bins=[48, 40], nreplicas=R, walkers=walkers)
    elif second == "distance":
        md = Metadynamics([("dihedral", PHI), ("distance", PAIR)], sigma=[0.35, 0.3], height=1.2, frequency=1, temperature=300.0,
                          bias_factor=bias_factor, grid_min=[None, 0.5], grid_max=[None, 6.0], grid_bins=[48, 40], nreplicas=R,
                          walkers=walkers)
    else:  # one CV: the distance alone
        md = Metadynamics(("distance", PAIR), sigma=0.3, height=1.2, frequency=1, temperature=300.0, bias_factor=bias_factor,
                          grid_min=0.5, grid_max=6.0, grid_bins=40, nreplicas=R, walkers=walkers)
    return pos, np.full(3, L), mass, md


def moved(pos, k, L=20.0, seed=3, amp=0.06):
    """The positions of deposition k: every atom displaced by up to `amp` Å per component (the bond angles of the chain stay
    within [60, 120] degrees from their [65, 115]), wrapped into the box."""
    rng = np.random.default_rng(seed + 1000 * k)
    return np.mod(pos + rng.uniform(-amp, amp, pos.shape), L)


def interp_magnitude(md, grid, s):
    """sum |term| of what `md.interp` adds up: (for V, for dV [ncv])."""
    k0 = locate(md.lo[0], md.h[0], int(md.nodes[0]), md.periodic[0], s[0])
    v0, d0 = hermite_basis(k0[2], md.h[0])
    if md.ncv == 1:
        mv = sum(abs(v0[a, 0] * grid[k][0]) + abs(v0[a, 1] * grid[k][1]) for a, k in enumerate(k0[:2]))
        md_ = sum(abs(d0[a, 0] * grid[k][0]) + abs(d0[a, 1] * grid[k][1]) for a, k in enumerate(k0[:2]))
        return mv, np.array([md_])
    k1 = locate(md.lo[1], md.h[1], int(md.nodes[1]), md.periodic[1], s[1])
    v1, d1 = hermite_basis(k1[2], md.h[1])
    mv = ma = mb = 0.0
    for a, ka in enumerate(k0[:2]):
        for b, kb in enumerate(k1[:2]):
            nd = np.abs(grid[ka, kb])
            for (p, q), val in zip(((0, 0), (1, 0), (0, 1), (1, 1)), nd):
                mv += abs(v0[a, p] * v1[b, q]) * val
                ma += abs(d0[a, p] * v1[b, q]) * val
                mb += abs(v0[a, p] * d1[b, q]) * val
    return mv, np.array([ma, mb])


def gaussian_sum(md, hills, s):
    """The analytic sum of Gaussians (V, dV [ncv]) at CV values s: hills [n, ncv + 1] = (s0..., w), minimum image on a
    periodic CV."""
    V, dV = 0.0, np.zeros(md.ncv)
    for hl in hills:
        d = np.asarray(s, dtype=np.float64) - hl[: md.ncv]
        for c in range(md.ncv):
            if md.periodic[c]:
                d[c] -= 2.0 * np.pi * np.rint(d[c] / (2.0 * np.pi))
        e = hl[md.ncv] * np.exp(-np.sum(d * d / (2.0 * md.sigma[: md.ncv] ** 2)))
        V += e
        dV += -d / md.sigma[: md.ncv] ** 2 * e
    return V, dV


# ----------------------------------------------------------------------------- the splitting, on the host
class BiasToy(RS.Toy):
    """The toy of tests/_restraints.py (8 particles in open space under a harmonic "physical" force) with a 1-D tabulated bias
    on the distance between particles 0 and 5 in the place of its restraints: `f_restraint` is the model's bias force on the
    grid as it stands, so `run_inside` / `run_impulse` of _restraints integrate under it unchanged."""

    def __init__(self, seed=5):
        super().__init__(seed)
        self.md = Metadynamics(("distance", (0, 5)), sigma=0.3, height=4.0, frequency=4, temperature=300.0, bias_factor=8.0,
                               grid_min=0.3, grid_max=15.3, grid_bins=100)
        r = np.linalg.norm(self.x0[0] - self.x0[5])
        assert 1.0 < r < 14.0
        grid = self.md.grid.copy()
        for off, w in ((0.25, 6.0), (-0.45, 3.0)):  # two hills beside the start: a bias force of several kcal/mol/Å
            grid[0] += self.md.gauss_terms(np.array([r + off]), w)
        self.grid0 = grid
        self.grid = grid.copy()

    def f_restraint(self, x):
        return self.md.energy_forces(x[None], self.box, self.grid)[1][0]

    def deposit(self, x):
        self.grid, rows = self.md.deposit_model(x[None], self.box, self.grid)
        return rows


def run_cut_depositing(run, toy, cuts, dt, gamma, **kw):
    """`_restraints.run_cut` with a deposition between the calls (none after the last): the force buffer a call leaves was
    evaluated on the grid of before the deposition, as `Integrator.step` leaves `systems.forces`."""
    vc = np.sqrt(2.0 * gamma * 0.596 * dt / toy.mass)[:, None] if gamma != 0.0 else 0.0
    toy.grid = toy.grid0.copy()
    x, v = toy.x0.copy(), toy.v0.copy()
    f = toy.f_phys(x) + toy.f_restraint(x)
    step0, hills = 0, []
    for k, n in enumerate(cuts):
        x, v, f = run(toy, x, v, f, n, step0, dt, gamma, vc, **kw)
        step0 += n
        if k + 1 < len(cuts):
            hills.append(toy.deposit(x))
    return x, v, f, hills
