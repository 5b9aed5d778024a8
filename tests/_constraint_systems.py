"""A seeded synthetic topology that holds every unit kind of the constrained MD step (csrc/md_cons.hip, md_step_cons_kernel)
in one context: free ions, TIP3P waters, H2S-like "waters" (32.06 amu, 1.34 A, 92 degrees: `find_constraints` takes any heavy
atom with exactly two hydrogens for a rigid three-atom unit), and X-H clusters of 1, 2, 3 and 4 hydrogens around heavy atoms
of different masses (C, N, O, S), some of the heavy atoms bonded to each other.

As tests/_bonded_systems.py: `build(size)` returns a `System` (a dict of `par_*` arrays for `GoldenParameters`, positions,
a cubic box).  Molecules sit on a lattice, randomly rotated, far enough apart that the start is tame; the atoms are numbered
by a random permutation, so that hydrogens do not follow their heavy atom, units interleave, and a unit's atoms fall into
different 64-atom blocks.  Bonds and angles carry ordinary force constants, LJ and charges are modest.

Sizes: SMALL is a few hundred atoms (a periodic box that algorithm="auto" runs all-pairs); LARGE has exactly
`CELLLIST_MIN_ATOMS` atoms, the smallest periodic context that "auto" gives the cell list (csrc/context.hip, tmdhip_create:
`cutoff > 0 && n >= 2048`; the box has well over three cells of cutoff + skin per edge)."""

from __future__ import annotations

import numpy as np

from _bonded_systems import System, _check_geometry, _rotation

TERMS = ["bonds", "angles", "lj", "electrostatics"]
FORCE_KW = dict(cutoff=9.0, switch_dist=7.5, rfa=True)
CELLLIST_MIN_ATOMS = 2048
SMALL, LARGE = "small", "large"
SPACING = 7.0  # lattice constant (A): the largest molecule reaches 2.3 A from its centre

TET = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]]) / np.sqrt(3.0)
THETA_TET = float(np.arccos(-1.0 / 3.0))
M_H = 1.008
M = {"C": 12.011, "N": 14.007, "O": 15.9994, "S": 32.06, "Na": 22.98977, "Cl": 35.453}
# LJ classes (sigma, epsilon): carbon, nitrogen / oxygen, sulfur, hydrogen, ions
LJ_CLASSES = np.array([[3.4, 0.10], [3.15, 0.15], [3.6, 0.25], [0.4, 0.03], [2.6, 0.05]])
LJ_OF = {"C": 0, "N": 1, "O": 1, "S": 2, "H": 3, "Na": 4, "Cl": 4}
Q_HEAVY_PER_H = -0.2  # charges: +0.2 on every cluster hydrogen, -0.2 per hydrogen on its heavy atom


class _Mol:
    def __init__(self):
        self.el, self.pos, self.q, self.bonds, self.angles = [], [], [], [], []

    def atom(self, el, pos, q=0.0):
        self.el.append(el)
        self.pos.append(np.asarray(pos, dtype=np.float64))
        self.q.append(q)
        return len(self.el) - 1

    def bond(self, i, j, k0, req):
        self.bonds.append((i, j, k0, req))

    def hydrogens(self, x, dirs, req, k0=340.0):
        """Hydrogens on atom x along `dirs`, at the bond length; the heavy atom takes the opposite charge."""
        out = []
        for d in dirs:
            h = self.atom("H", self.pos[x] + req * np.asarray(d), 0.2)
            self.q[x] += Q_HEAVY_PER_H
            self.bond(x, h, k0, req)
            out.append(h)
        return out

    def angles_around(self, x, k0=45.0):
        nb = [j if i == x else i for i, j, _, _ in self.bonds if x in (i, j)]
        for a in range(len(nb)):
            for b in range(a + 1, len(nb)):
                self.angles.append((nb[a], x, nb[b], k0, THETA_TET))


def _three_site(el, req, theta, k_bond, k_angle, q_h):
    m = _Mol()
    o = m.atom(el, np.zeros(3), -2 * q_h)
    for s in (1, -1):
        h = m.atom("H", req * np.array([s * np.sin(theta / 2), np.cos(theta / 2), 0.0]), q_h)
        m.bond(o, h, k_bond, req)
    m.angles.append((1, 0, 2, k_angle, theta))
    return m


def tip3p():
    return _three_site("O", 0.9572, np.deg2rad(104.52), 450.0, 55.0, 0.417)


def h2s():
    return _three_site("S", 1.34, np.deg2rad(92.0), 300.0, 40.0, 0.15)


def _xh4(el, req):  # NH4+ / CH4 class: four hydrogens, the `default:` (NA = 5) branch
    m = _Mol()
    x = m.atom(el, np.zeros(3))
    m.hydrogens(x, TET, req)
    m.angles_around(x)
    return m


def _two_heavy(el_b, d_ab, nh_b, req_b, el_a="C", nh_a=3, req_a=1.09):
    """A(H nh_a)-B(H nh_b): methanol (3, 1), methylamine (3, 2), methanethiol (3, 1), methylammonium (3, 3) classes; the
    hydrogens of B are staggered against those of A."""
    m = _Mol()
    a = m.atom(el_a, np.zeros(3))
    b = m.atom(el_b, d_ab * TET[0])
    m.bond(a, b, 300.0, d_ab)
    m.hydrogens(a, TET[1:1 + nh_a], req_a)
    m.hydrogens(b, -TET[1:1 + nh_b], req_b)
    m.angles_around(a), m.angles_around(b)
    return m


def _ethanol():  # CH3-CH2-OH: clusters of 3, 2 and 1 hydrogens on a chain of three heavy atoms
    m = _Mol()
    c1 = m.atom("C", np.zeros(3))
    c2 = m.atom("C", 1.53 * TET[0])
    o = m.atom("O", m.pos[c2] - 1.43 * TET[1])
    m.bond(c1, c2, 300.0, 1.53), m.bond(c2, o, 320.0, 1.43)
    m.hydrogens(c1, TET[1:], 1.09)
    m.hydrogens(c2, -TET[2:], 1.09)
    m.hydrogens(o, TET[:1], 0.96, k0=450.0)
    for x in (c1, c2, o):
        m.angles_around(x)
    return m


# (name, builder, cluster sizes) — every cluster size on two different heavy masses
TEMPLATES = [
    ("methanol", lambda: _two_heavy("O", 1.43, 1, 0.96), [3, 1]),
    ("methylamine", lambda: _two_heavy("N", 1.47, 2, 1.01), [3, 2]),
    ("methanethiol", lambda: _two_heavy("S", 1.82, 1, 1.34), [3, 1]),
    ("methylammonium", lambda: _two_heavy("N", 1.50, 3, 1.03), [3, 3]),
    ("ethanol", _ethanol, [3, 2, 1]),
    ("ammonium", lambda: _xh4("N", 1.03), [4]),
    ("methane", lambda: _xh4("C", 1.09), [4]),
]


def build(size=SMALL, seed=7):
    """meta: `counts` (molecules per kind), `nwaters`, `nclusters`, `cluster_sizes` (hydrogens per cluster, sorted),
    `nions`, `nconstraints`, `kind` (per atom: "ion", "tip3p", "h2s", "cluster")."""
    rng = np.random.default_rng(seed)
    natoms = 260 if size == SMALL else CELLLIST_MIN_ATOMS
    per = 2 if size == SMALL else 20  # molecules of every cluster template
    nw3, nws = (24, 12) if size == SMALL else (200, 100)
    mols = [(name, fn()) for name, fn, _ in TEMPLATES for _ in range(per)]
    mols += [("tip3p", tip3p()) for _ in range(nw3)] + [("h2s", h2s()) for _ in range(nws)]
    mols = [mols[i] for i in rng.permutation(len(mols))]
    nmolat = sum(len(m.el) for _, m in mols)
    nions = natoms - nmolat
    assert nions >= 8, (size, nmolat)
    side = int(np.ceil((len(mols) + nions) ** (1 / 3)))
    L = side * SPACING
    sites = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), -1).reshape(-1, 3) * SPACING + 0.5 * SPACING
    sites = sites[rng.permutation(len(sites))]
    pos, el, q, kind, bonds, angles = [], [], [], [], [], []
    for (name, m), c in zip(mols, sites):
        base = len(pos)
        x = np.array(m.pos)
        x = (x - x.mean(axis=0)) @ _rotation(rng).T + c + rng.uniform(-0.3, 0.3, 3)
        pos += list(x)
        el += m.el
        q += m.q
        kind += [name if name in ("tip3p", "h2s") else "cluster"] * len(x)
        bonds += [(base + i, base + j, k0, r) for i, j, k0, r in m.bonds]
        angles += [(base + i, base + j, base + k, k0, t) for i, j, k, k0, t in m.angles]
    for s, c in enumerate(sites[len(mols):len(mols) + nions]):
        pos.append(c + rng.uniform(-0.5, 0.5, 3))
        el.append("Na" if s % 2 == 0 else "Cl")
        q.append(0.5 if s % 2 == 0 else -0.5)
        kind.append("ion")
    n = len(pos)
    assert n == natoms
    perm = rng.permutation(n)  # new index of old atom i
    inv = np.argsort(perm)
    mass = np.array([M_H if e == "H" else M[e] for e in el])
    g = {"par_charges": np.array(q)[inv], "par_masses": mass[inv][:, None], "par_types": np.array([LJ_OF[e] for e in el])[inv],
         "par_nonbonded_params": LJ_CLASSES.copy()}
    for key, rows, w in (("bond", bonds, 2), ("angle", angles, 3)):
        order = rng.permutation(len(rows))
        g[f"par_{key}_idx"] = np.array([[perm[a] for a in rows[t][:w]] for t in order], dtype=np.int64)
        g[f"par_{key}_map"] = np.stack([np.arange(len(rows)), np.arange(len(rows))], 1)
        g[f"par_{key}_params"] = np.array([rows[t][w:] for t in order], dtype=np.float64)
    sizes = sorted(s for name, _ in mols for tn, _, cl in TEMPLATES if tn == name for s in cl)
    counts = {name: sum(1 for nm, _ in mols if nm == name) for name in [t[0] for t in TEMPLATES] + ["tip3p", "h2s"]}
    meta = dict(perm=perm, counts=counts, nwaters=nw3 + nws, nclusters=len(sizes), cluster_sizes=sizes, nions=nions,
                nconstraints=3 * (nw3 + nws) + sum(sizes), kind=np.array(kind)[inv])
    s = System(f"constraints-{size}", g, np.array(pos)[inv], np.full(3, L), meta)
    _check_geometry(s, min_nonbonded=2.0)
    return s
