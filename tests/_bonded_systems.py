"""Seeded synthetic topologies that reach every branch of the bonded evaluators (csrc/bonded.hip, bonded_math.h,
md_loop.hip, md_step.h, pair_generic.hip).

Each builder returns a `System`: a dict of `par_*` arrays in the layout of tests/golden/*.npz (so `GoldenParameters`
rebuilds the `Parameters` duck type from it), unwrapped positions and a cubic box.  A system is small molecules on a
lattice, randomly rotated, with free ions in between; the atoms are numbered by a random permutation, so that the atoms
of a molecule fall into different 64-atom blocks.  Molecules on the lattice sites next to a box face straddle it, some
of them with their outside atoms wrapped back into the box, and some atoms sit one or two box lengths outside.

Record counts follow `set_bonded` (bonded.hip): `records_per_atom` mirrors them, and every builder asserts on which side
of the light / heavy threshold (`kAtomCentricLimit` = 8 records per atom) it lands.
"""

from __future__ import annotations

from dataclasses import dataclass, field
from math import pi

import numpy as np
import torch

from oracle import torchmd_oracle as orc

from _golden import GoldenParameters

BONDED = ["bonds", "angles", "dihedrals", "impropers", "1-4"]
ALL_TERMS = BONDED + ["electrostatics", "lj"]
ATOM_CENTRIC_LIMIT = 8  # kAtomCentricLimit in csrc/bonded.hip
SMALL, LARGE = "small", "large"  # <= 2048 atoms (all-pairs, ride rows) / 4-8k atoms (cell list, lean fp32 kernel)

# LJ classes (sigma, epsilon): a handful, well under the lean kernel's 32
LJ_CLASSES = np.array([[1.6, 0.05], [2.0, 0.10], [2.4, 0.08], [1.8, 0.12], [2.2, 0.06]])


@dataclass
class System:
    name: str
    g: dict  # par_* arrays (float64 parameters) as in tests/golden/*.npz
    pos: np.ndarray  # [N, 3] float64, unwrapped
    box: np.ndarray  # [3]
    meta: dict = field(default_factory=dict)

    @property
    def natoms(self):
        return len(self.pos)

    def par(self, dtype=torch.float64):
        return GoldenParameters(self.g, dtype)

    def rounded(self, dtype):
        """The same system with every real input rounded to `dtype` (stored as float64 again): what an fp32 context sees,
        handed to the fp64 oracle."""
        def rnd(a):
            a = np.asarray(a)
            return a.astype(np.float32).astype(np.float64) if dtype == torch.float32 and a.dtype.kind == "f" else a
        return System(self.name, {k: rnd(v) for k, v in self.g.items()}, rnd(self.pos), rnd(self.box), self.meta)

    def with_tables(self, **keep):
        """A copy whose tables keep only the rows selected by boolean masks, e.g. `with_tables(bond=mask)`; a table set
        to None is removed."""
        g = dict(self.g)
        for name, mask in keep.items():
            for k in ("idx", "map", "params"):
                g.pop(f"par_{name}_{k}", None)
            if mask is None:
                continue
            idx, mp, prm = self.g[f"par_{name}_idx"], self.g[f"par_{name}_map"], self.g[f"par_{name}_params"]
            rows = np.flatnonzero(mask)
            renum = -np.ones(len(idx), dtype=np.int64)
            renum[rows] = np.arange(len(rows))
            m = mp[renum[mp[:, 0]] >= 0].copy()
            m[:, 0] = renum[m[:, 0]]
            g[f"par_{name}_idx"], g[f"par_{name}_map"], g[f"par_{name}_params"] = idx[rows], m, prm
        return System(self.name, g, self.pos, self.box, self.meta)


def records_per_atom(par, terms):
    """Per-atom record count of `set_bonded` (bonded.hip) for a Parameters duck type: one record per (term, atom) for the
    requested tables, except bonds with k0 == 0 (none) and 1-4 pairs (only with "lj" or "electrostatics" requested)."""
    terms = [t.lower() for t in terms]
    n = len(par.charges)
    cnt = np.zeros(n, dtype=np.int64)

    def add(idx):
        np.add.at(cnt, np.asarray(idx.cpu(), dtype=np.int64).reshape(-1), 1)

    if "bonds" in terms and par.bond_params is not None:
        prm = par.bond_params["params"][par.bond_params["map"][:, 1]]
        add(par.bond_params["idx"][(prm[:, 0] != 0).cpu()])
    if "angles" in terms and par.angle_params is not None:
        add(par.angle_params["idx"])
    if "dihedrals" in terms and par.dihedral_params is not None:
        add(par.dihedral_params["idx"])
    if "impropers" in terms and par.improper_params is not None:
        add(par.improper_params["idx"])
    p14 = par.nonbonded_14_params
    if "1-4" in terms and p14 is not None and ("lj" in terms or "electrostatics" in terms):
        add(p14["idx"])
    return cnt


def slot_kinds(par, terms, atom):
    """The kinds of atom `atom`'s records in slot order (set_bonded fills them table by table, rows in order)."""
    out = []
    for kind, tab in (("bonds", par.bond_params), ("angles", par.angle_params), ("dihedrals", par.dihedral_params),
                      ("impropers", par.improper_params), ("1-4", par.nonbonded_14_params)):
        if kind not in terms or tab is None:
            continue
        if kind == "1-4" and "lj" not in terms and "electrostatics" not in terms:
            continue
        idx = np.asarray(tab["idx"].cpu())
        live = np.ones(len(idx), bool)
        if kind == "bonds":
            live = np.asarray(tab["params"][tab["map"][:, 1]][:, 0].cpu()) != 0
        out += [kind] * int(((idx == atom) & live[:, None]).any(axis=1).sum())
    return out


# ----------------------------------------------------------------------------- geometry helpers
def _rotation(rng):
    q = rng.standard_normal(4)
    q /= np.linalg.norm(q)
    a, b, c, d = q
    return np.array([[a * a + b * b - c * c - d * d, 2 * (b * c - a * d), 2 * (b * d + a * c)],
                     [2 * (b * c + a * d), a * a - b * b + c * c - d * d, 2 * (c * d - a * b)],
                     [2 * (b * d - a * c), 2 * (c * d + a * b), a * a - b * b - c * c + d * d]])


def _place(a, b, c, bond, angle, torsion):
    """Natural-extension placement: atom d with |cd| = bond, angle bcd, torsion abcd (radians)."""
    bc = c - b
    bc /= np.linalg.norm(bc)
    nrm = np.cross(b - a, bc)
    nrm /= np.linalg.norm(nrm)
    m = np.stack([bc, np.cross(nrm, bc), nrm], axis=1)
    d2 = np.array([-bond * np.cos(angle), bond * np.sin(angle) * np.cos(torsion), bond * np.sin(angle) * np.sin(torsion)])
    return c + m @ d2


def _chain(rng, n):
    while True:
        p = [np.zeros(3), np.array([1.5, 0, 0])]
        p.append(p[1] + 1.5 * np.array([-np.cos(1.9), np.sin(1.9), 0]))
        while len(p) < n:
            p.append(_place(p[-3], p[-2], p[-1], rng.uniform(1.4, 1.6), rng.uniform(1.85, 2.05), rng.uniform(-pi, pi)))
        p = np.array(p)
        if n < 5 or np.linalg.norm(p[4] - p[0]) > 2.6:  # (the 1-5 pair is not excluded)
            return p - p.mean(axis=0)


def _angle(p, i, j, k):
    u, v = p[i] - p[j], p[k] - p[j]
    return float(np.arccos(np.clip(u @ v / np.linalg.norm(u) / np.linalg.norm(v), -1, 1)))


class _Builder:
    """Collects molecules (local coordinates + terms) and ions, then numbers, places and permutes them."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.mols = []  # dict(pos, types, charges, masses, bonds, angles, dihedrals, impropers, rotate)

    # -- terms.  Bond / angle parameters sit near the geometry; torsions get 1-3 Fourier terms
    def bond(self, m, i, j, k0=None, d0=None):
        d = np.linalg.norm(m["pos"][i] - m["pos"][j])
        m["bonds"].append((i, j, self.rng.uniform(100, 300) if k0 is None else k0,
                           d + self.rng.uniform(-0.05, 0.05) if d0 is None else d0))

    def angle(self, m, i, j, k, k0=None, th0=None):
        th = _angle(m["pos"], i, j, k)
        m["angles"].append((i, j, k, self.rng.uniform(20, 60) if k0 is None else k0,
                            th + self.rng.uniform(-0.15, 0.15) if th0 is None else th0))

    def dihedral(self, m, i, j, k, l, nterms=None):
        nterms = int(self.rng.integers(1, 4)) if nterms is None else nterms
        pers = self.rng.choice([1, 2, 3, 4], size=nterms, replace=False)
        rows = [(self.rng.uniform(0.1, 2.0), self.rng.choice([0.0, pi, self.rng.uniform(-pi, pi)]), float(p)) for p in pers]
        m["dihedrals"].append(((i, j, k, l), rows))

    def improper(self, m, i, j, k, l):
        m["impropers"].append(((i, j, k, l), [(self.rng.uniform(1.0, 10.0), pi, 2.0)]))

    def molecule(self, pos, types, rotate=True):
        n = len(pos)
        m = dict(pos=np.asarray(pos, float), types=list(types), charges=list(self.rng.uniform(-0.5, 0.5, n)),
                 masses=list(self.rng.uniform(1.0, 16.0, n)), bonds=[], angles=[], dihedrals=[], impropers=[], rotate=rotate)
        self.mols.append(m)
        return m

    # -- templates
    def chain(self, n, improper=True):
        """n = 4 or 5 atoms in a row: bonds, angles and dihedrals along it (1-4 pairs = the dihedrals' ends), an improper
        over the first four.  Record counts (with 1-4): chain4 [5, 6, 6, 5]; chain5 [5, 8, 8, 8, 4] (atom 1: two bonds,
        two angles, two dihedrals, the improper and a 1-4 pair, in that slot order); chain5 without the improper
        [4, 7, 7, 7, 4]."""
        m = self.molecule(_chain(self.rng, n), self.rng.integers(0, 4, n))
        for i in range(n - 1):
            self.bond(m, i, i + 1)
        for i in range(n - 2):
            self.angle(m, i, i + 1, i + 2)
        for i in range(n - 3):
            self.dihedral(m, i, i + 1, i + 2, i + 3)
        if improper:
            self.improper(m, 0, 1, 2, 3)
        return m

    def triatomic(self):  # [2, 3, 2]
        p = np.array([[0.0, 0, 0], [1.0, 0, 0], [1.0 - np.cos(1.9), np.sin(1.9), 0]])
        m = self.molecule(p - p.mean(axis=0), self.rng.integers(0, 4, 3))
        self.bond(m, 0, 1), self.bond(m, 0, 2), self.angle(m, 1, 0, 2)
        return m

    def diatomic(self, k0=None):  # [1, 1]; k0 = 0: no record at all (set_bonded drops it)
        m = self.molecule(np.array([[-0.6, 0, 0], [0.6, 0, 0]]), self.rng.integers(0, 4, 2))
        self.bond(m, 0, 1, k0=k0)
        return m

    def hub(self, spokes=16, tails=4):
        """A star: the centre is bonded to `spokes` atoms, every pair of spokes makes an angle at the centre
        (16 spokes: 16 bonds + 120 angles), `tails` spokes carry one more atom, and torsions tail-spoke-centre-spoke run
        through the centre (with their 1-4 pairs): > 128 entries on the centre, three passes of a 64-lane wave."""
        k = np.arange(spokes) + 0.5
        z = 1 - 2 * k / spokes
        phi = pi * (1 + 5 ** 0.5) * k
        sp = 2.2 * np.stack([np.sqrt(1 - z * z) * np.cos(phi), np.sqrt(1 - z * z) * np.sin(phi), z], axis=1)
        p = [np.zeros(3)] + list(sp)
        tail_of = {}
        for t in range(tails):
            s = 1 + t * (spokes // tails)
            far = sp[(s - 1 + spokes // 2) % spokes]
            p.append(_place(np.zeros(3) + far, np.zeros(3), p[s], 1.3, 2.6, pi / 2 + t))
            tail_of[s] = len(p) - 1
        m = self.molecule(np.array(p), [4] * len(p))
        for s in range(1, spokes + 1):
            self.bond(m, 0, s, k0=self.rng.uniform(100, 300))
        for a in range(1, spokes + 1):
            for b in range(a + 1, spokes + 1):
                self.angle(m, a, 0, b, k0=self.rng.uniform(2, 10))
        for s, t in tail_of.items():
            self.bond(m, s, t)
            self.angle(m, 0, s, t)
            partners = [b for b in range(1, spokes + 1) if b != s and 1.0 < _angle(m["pos"], s, 0, b) < 2.1][:2]
            for b in partners:
                self.dihedral(m, t, s, 0, b)
        return m

    # -- assembly
    def build(self, name, n_target, spacing, straddle_wrap=True, check=True):
        rng = self.rng
        nmol = len(self.mols)
        side = int(np.ceil(nmol ** (1 / 3)))
        L = side * spacing
        sites = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), -1).reshape(-1, 3) * spacing + 0.3
        sites = sites[rng.permutation(len(sites))[:nmol]]
        pos, types, q, mass = [], [], [], []
        tabs = {k: [] for k in ("bond", "angle", "dihedral", "improper")}
        mol_of = []
        for mi, (m, c) in enumerate(zip(self.mols, sites)):
            base = len(pos)
            x = m["pos"] @ _rotation(rng).T if m["rotate"] else m["pos"]
            x = x + (c + rng.uniform(-0.3, 0.3, 3) if m["rotate"] else np.round(c * 4) / 4)
            pos += list(x)
            types += list(m["types"])
            q += list(m["charges"])
            mass += list(m["masses"])
            mol_of += [mi] * len(x)
            tabs["bond"] += [((base + i, base + j), [(k0, d0)]) for i, j, k0, d0 in m["bonds"]]
            tabs["angle"] += [((base + i, base + j, base + k), [(k0, t0)]) for i, j, k, k0, t0 in m["angles"]]
            for kind in ("dihedral", "improper"):
                tabs[kind] += [(tuple(base + a for a in ix), rows) for ix, rows in m[kind + "s"]]
        nmolat = len(pos)
        # ions in the gaps between the molecules (cell centres of the lattice)
        nions = max(0, n_target - nmolat)
        free = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), -1).reshape(-1, 3) * spacing + 0.3 + spacing / 2
        assert nions <= len(free), (name, nions, len(free))
        pos += list(free[rng.permutation(len(free))[:nions]] + rng.uniform(-0.5, 0.5, (nions, 3)))
        types += list(rng.integers(0, 4, nions))
        q += list(rng.uniform(-0.5, 0.5, nions))
        mass += list(rng.uniform(10.0, 40.0, nions))
        mol_of += [-1] * nions
        pos, mol_of = np.array(pos), np.array(mol_of)
        # straddling molecules: the atoms of molecules at the faces that lie outside are wrapped back (half of them);
        # then some atoms are moved one box length out, and a few ions two
        box = np.full(3, L)
        out = (pos < 0) | (pos >= L)
        if straddle_wrap:
            wrap_mol = rng.random(nmol) < 0.5
            sel = out.any(axis=1) & (mol_of >= 0) & wrap_mol[np.maximum(mol_of, 0)]
            pos[sel] -= np.floor(pos[sel] / L) * L
        movable = np.flatnonzero(mol_of >= 0)
        shift = rng.choice(movable, size=len(movable) // 10, replace=False)
        pos[shift] += L * rng.choice([-1, 1], size=(len(shift), 3)) * (rng.random((len(shift), 3)) < 0.5)
        ions = np.flatnonzero(mol_of < 0)
        if len(ions):
            far = rng.choice(ions, size=max(1, len(ions) // 20), replace=False)
            pos[far] += 2 * L * rng.choice([-1, 1], size=(len(far), 3))
        # random numbering
        n = len(pos)
        perm = rng.permutation(n)  # new index of old atom i
        inv = np.argsort(perm)
        g = {"par_charges": np.array(q)[inv], "par_masses": np.array(mass)[inv][:, None], "par_types": np.array(types)[inv],
             "par_nonbonded_params": LJ_CLASSES.copy()}
        for kind, rows in tabs.items():
            if not rows:
                continue
            order = rng.permutation(len(rows))  # table rows in random order too
            idx = np.array([[perm[a] for a in rows[t][0]] for t in order], dtype=np.int64)
            terms = [(ti, r) for ti, t in enumerate(order) for r in rows[t][1]]
            mp_order = rng.permutation(len(terms)) if kind in ("dihedral", "improper") else np.arange(len(terms))
            prm = np.array([terms[k][1] for k in mp_order], dtype=np.float64)
            mp = np.array([[terms[k][0], j] for j, k in enumerate(mp_order)], dtype=np.int64)
            g[f"par_{kind}_idx"], g[f"par_{kind}_map"], g[f"par_{kind}_params"] = idx, mp, prm
        if "par_dihedral_idx" in g:  # 1-4 pairs: the ends of the dihedrals (one row each, as Parameters builds them)
            ends = g["par_dihedral_idx"][:, [0, 3]]
            s, e = LJ_CLASSES[g["par_types"][ends[:, 0]]], LJ_CLASSES[g["par_types"][ends[:, 1]]]
            sig6 = (0.5 * (s[:, 0] + e[:, 0])) ** 6
            eps4 = 4 * np.sqrt(s[:, 1] * e[:, 1])
            g["par_nonbonded_14_idx"] = ends.copy()
            g["par_nonbonded_14_map"] = np.stack([np.arange(len(ends)), np.arange(len(ends))], 1)
            g["par_nonbonded_14_params"] = np.stack([eps4 * sig6 * sig6, eps4 * sig6, np.full(len(ends), 2.0),
                                                     np.full(len(ends), 1.2)], 1)
        sysm = System(name, g, pos[inv], box, {})
        sysm.meta["perm"] = perm
        sysm.meta["mol_of"] = mol_of[inv]
        if check:
            _check_geometry(sysm)
        return sysm


def _check_geometry(s, min_nonbonded=1.9):
    """No close non-excluded contact, every angle of the regular set well away from 0 and pi, torsions well defined."""
    par = s.par()
    pos = torch.tensor(s.pos)
    box = torch.tensor(s.box)
    pairs = orc.candidate_pairs(s.pos, s.box, min_nonbonded, orc.exclusion_pairs(par))
    assert len(pairs) == 0, (s.name, "close contact", pairs[:4], s.meta["mol_of"][pairs[:4]] if "mol_of" in s.meta else None)
    skip = s.meta.get("linear_angles", np.zeros(0, dtype=np.int64))
    if par.angle_params is not None:
        idx = par.angle_params["idx"]
        _, _, r21 = orc.pair_geometry(pos, idx[:, [0, 1]], box)
        _, _, r23 = orc.pair_geometry(pos, idx[:, [2, 1]], box)
        c = (r21 * r23).sum(1) / r21.norm(dim=1) / r23.norm(dim=1)
        sn = torch.sqrt(1 - c * c).numpy()
        regular = np.ones(len(sn), bool)
        regular[skip] = False
        assert sn[regular].min() > 0.05, (s.name, sn[regular].min())
    for tab in (par.dihedral_params, par.improper_params):
        if tab is None:
            continue
        idx = tab["idx"]
        for a, b, c in ((0, 1, 2), (1, 2, 3)):
            _, _, u = orc.pair_geometry(pos, idx[:, [a, b]], box)
            _, _, v = orc.pair_geometry(pos, idx[:, [c, b]], box)
            sn = torch.cross(u, v, dim=1).norm(dim=1) / u.norm(dim=1) / v.norm(dim=1)
            assert sn.min().item() > 0.2, (s.name, "torsion with (nearly) collinear atoms")


def torsion_phi(s, table):
    """phi of every torsion of `table` ("dihedral" / "improper") in the oracle's fp64 arithmetic (forces.py:542-554)."""
    pos, box = torch.tensor(s.pos), torch.tensor(s.box)
    idx = torch.tensor(s.g[f"par_{table}_idx"])
    _, _, r12 = orc.pair_geometry(pos, idx[:, [0, 1]], box)
    _, _, r23 = orc.pair_geometry(pos, idx[:, [1, 2]], box)
    _, _, r34 = orc.pair_geometry(pos, idx[:, [2, 3]], box)
    cA, cB = torch.cross(r12, r23, dim=1), torch.cross(r23, r34, dim=1)
    cC = torch.cross(r23, cA, dim=1)
    uB = cB / cB.norm(dim=1, keepdim=True)
    return (-torch.atan2((cC * uB).sum(1) / cC.norm(dim=1), (cA * uB).sum(1) / cA.norm(dim=1))).numpy()


def harmonic_offsets(s, table):
    """phi - phi0 of every term of a harmonic table before the +-2 pi wrap, and after it."""
    phi = torsion_phi(s, table)
    mp, prm = s.g[f"par_{table}_map"], s.g[f"par_{table}_params"]
    raw = phi[mp[:, 0]] - prm[mp[:, 1], 1]
    wrapped = np.where(raw < -pi, raw + 2 * pi, np.where(raw > pi, raw - 2 * pi, raw))
    return raw, wrapped


# clearance of |phi - phi0| from pi (where the harmonic force jumps): ~1e-3 rad covers fp32 round-off of phi
WRAP_CLEARANCE = 2e-3


def _assert_light(s, heavy=False):
    par = s.par()
    for terms in (ALL_TERMS, BONDED):
        c = records_per_atom(par, terms).max()
        assert (c > ATOM_CENTRIC_LIMIT) == heavy, (s.name, terms, c)


def _size(size, small, large):
    return small if size == SMALL else large


# ----------------------------------------------------------------------------- systems
def _light_molecules(b, nmol):
    kinds = ["chain5", "chain5-noimp", "chain4", "tri", "di", "di0"]
    weights = np.array([4, 2, 2, 2, 1, 0.3])
    for k in b.rng.choice(kinds, size=nmol, p=weights / weights.sum()):
        if k == "chain5":
            b.chain(5)
        elif k == "chain5-noimp":
            b.chain(5, improper=False)
        elif k == "chain4":
            b.chain(4)
        elif k == "tri":
            b.triatomic()
        else:
            b.diatomic(k0=0.0 if k == "di0" else None)
    b.chain(5), b.chain(4), b.diatomic(0.0)  # every record count 0..8 present whatever the draw


def light_full(size=SMALL, seed=1, plus_one=False):
    """Light topology with exactly 8 records on the fullest atoms: all five kinds, some atom with each count 0..8, and
    an atom whose slots 4-7 hold dihedral, dihedral, improper, 1-4 (chain5's atom 1).  `plus_one`: the same system with one
    more bond on one 8-record atom (chain5's atom 2 to atom 0): 9 records, the heavy scheme."""
    b = _Builder(seed)
    nmol = _size(size, 380, 1150)
    _light_molecules(b, nmol)
    if plus_one:
        m = next(m for m in b.mols if len(m["pos"]) == 5 and m["impropers"])
        b.bond(m, 0, 2, k0=50.0)
    s = b.build("light-plus-one" if plus_one else "light-full", _size(size, 2000, 6000), 7.0)
    par = s.par()
    cnt = records_per_atom(par, ALL_TERMS)
    if plus_one:
        assert cnt.max() == ATOM_CENTRIC_LIMIT + 1 and (cnt > ATOM_CENTRIC_LIMIT).sum() == 1, np.bincount(cnt)
        assert records_per_atom(par, BONDED).max() == ATOM_CENTRIC_LIMIT + 1
    else:
        assert cnt.max() == ATOM_CENTRIC_LIMIT and set(range(ATOM_CENTRIC_LIMIT + 1)) <= set(cnt.tolist()), np.bincount(cnt)
        assert records_per_atom(par, BONDED).max() == ATOM_CENTRIC_LIMIT
        assert any(slot_kinds(par, ALL_TERMS, a)[4:] == ["dihedrals", "dihedrals", "impropers", "1-4"] for a in np.flatnonzero(cnt == 8))
    assert s.natoms <= 2048 if size == SMALL else 4000 <= s.natoms <= 8000
    _assert_light(s, heavy=plus_one)
    return s


def light_plus_one(size=SMALL, seed=1):
    return light_full(size, seed, plus_one=True)


def hub(size=SMALL, seed=2):
    """Star molecules (centre: 16 bonds, 120 angles, tail angles and torsions: > 128 entries) among light molecules."""
    b = _Builder(seed)
    for _ in range(_size(size, 6, 10)):
        b.hub()
    _light_molecules(b, _size(size, 340, 1100))
    b.mols = [b.mols[i] for i in b.rng.permutation(len(b.mols))]
    s = b.build("hub", _size(size, 2000, 6000), 7.5)
    cnt = records_per_atom(s.par(), BONDED)
    assert cnt.max() > 128 and (cnt > 128).sum() == _size(size, 6, 10), cnt.max()
    assert s.natoms <= 2048 if size == SMALL else 4000 <= s.natoms <= 8000
    _assert_light(s, heavy=True)
    return s


def harmonic(size=SMALL, seed=3, harmonic_dihedrals=False):
    """Impropers with per = 0 (CHARMM harmonic: the whole improper table) beside AMBER dihedrals; `harmonic_dihedrals`:
    one dihedral row with per = 0 too, which makes the whole dihedral table harmonic (torch.all(per > 0) per table).
    phi0 is drawn so that phi - phi0 falls past +-pi for some terms (the wrap) and never within WRAP_CLEARANCE of it."""
    b = _Builder(seed)
    _light_molecules(b, _size(size, 380, 1150))
    s = b.build("harmonic-dihedrals" if harmonic_dihedrals else "harmonic", _size(size, 2000, 6000), 7.0)
    rng = np.random.default_rng(seed + 100)
    g = s.g
    tables = ["improper"] + (["dihedral"] if harmonic_dihedrals else [])
    g["par_improper_params"][:, 0] = rng.uniform(2.0, 20.0, len(g["par_improper_params"]))
    g["par_improper_params"][:, 2] = 0.0
    if harmonic_dihedrals:
        g["par_dihedral_params"][rng.integers(len(g["par_dihedral_params"])), 2] = 0.0
    for t in tables:
        prm = g[f"par_{t}_params"]
        prm[:, 1] = rng.uniform(-pi, pi, len(prm))
        for _ in range(20):  # move phi0 of the few terms too close to the jump
            _, w = harmonic_offsets(s, t)
            bad = np.abs(np.abs(w) - pi) < 2 * WRAP_CLEARANCE
            if not bad.any():
                break
            rows = s.g[f"par_{t}_map"][bad, 1]
            prm[rows, 1] = rng.uniform(-pi, pi, len(rows))
    for t in tables:
        raw, w = harmonic_offsets(s, t)
        assert np.abs(np.abs(w) - pi).min() >= WRAP_CLEARANCE, t
        assert (raw > pi).sum() >= 3 and (raw < -pi).sum() >= 3, (t, (raw > pi).sum(), (raw < -pi).sum())
    par = s.par()
    assert not bool(torch.all(par.improper_params["params"][:, 2] > 0))
    assert bool(torch.all(par.dihedral_params["params"][:, 2] > 0)) != harmonic_dihedrals
    _assert_light(s)
    return s


def harmonic_dihedrals(size=SMALL, seed=3):
    return harmonic(size, seed, harmonic_dihedrals=True)


def near_cutoff_positions(dtype, cutoff, start, direction, offsets=(-2, -1, 0, 1, 2)):
    """Second atoms at distance cutoff + k ulps from `start` (k in offsets), in the oracle's own `dist` arithmetic
    (pair_geometry in `dtype`): the point start + cutoff * direction, nudged by a few ulps per coordinate until the
    distance lands on each offset.  Returns [len(offsets), 3] float64 positions exactly representable in dtype."""
    npdt = np.float32 if dtype == torch.float32 else np.float64
    c = npdt(cutoff)
    start = np.asarray(start, dtype=npdt)
    p0 = (start.astype(np.float64) + cutoff * np.asarray(direction)).astype(npdt)
    n = np.arange(-8, 9)
    grid = np.stack(np.meshgrid(n, n, n, indexing="ij"), -1).reshape(-1, 3)
    cand = (p0[None, :] + grid * np.spacing(np.abs(p0))[None, :]).astype(npdt)
    pos = torch.tensor(np.concatenate([start[None], cand]))
    idx = torch.stack([torch.zeros(len(cand), dtype=torch.int64), torch.arange(1, len(cand) + 1)], 1)
    d = orc.pair_geometry(pos, idx, None)[0].numpy()
    ulps = np.round((d.astype(np.float64) - float(c)) / float(np.spacing(c))).astype(np.int64)
    out = []
    for k in offsets:
        hit = np.flatnonzero((ulps == k) & (d == np.asarray(float(c) + k * float(np.spacing(c)), dtype=npdt)))
        assert len(hit), (k, np.unique(ulps))
        out.append(cand[hit[0]].astype(np.float64))
    return np.stack(out)


def edges(dtype=torch.float64, size=SMALL, seed=4, cutoff=9.0):
    """Angles within 1e-3 rad of linear and exactly linear (cos = -1 exactly: the clamp and sin = 0), each with
    theta0 = pi and theta0 != pi; bonds longer than the cutoff; bonds of length cutoff + k ulps (k = -2..2 in `dtype`),
    placed with the oracle's dist arithmetic.  meta: `linear_angles` / `near_linear_angles` (angle rows),
    `long_bonds` / `near_cutoff_bonds` (bond rows), `near_cutoff_offsets` (k of each near-cutoff bond)."""
    b = _Builder(seed)
    _light_molecules(b, _size(size, 380, 1150))
    rng = b.rng
    special = []
    for j in range(8):  # near-linear: theta = pi - delta, delta in [5e-4, 1e-3]
        dl = rng.uniform(5e-4, 1e-3)
        p = np.array([[1.2, 0, 0], [0, 0, 0], [-1.4 * np.cos(dl), 1.4 * np.sin(dl), 0]])
        m = b.molecule(p - p.mean(axis=0), rng.integers(0, 4, 3))
        b.bond(m, 0, 1), b.bond(m, 1, 2)
        b.angle(m, 0, 1, 2, k0=rng.uniform(20, 60), th0=pi if j % 2 == 0 else 2.6)
        special.append(("near_linear", m))
    for j in range(4):  # exactly linear, axis-aligned on a quarter-angstrom grid: |r21| = 1, |r23| = 2, cos = -1 exactly
        p = np.array([[1.0, 0, 0], [0, 0, 0], [-2.0, 0, 0]])[:, np.roll([0, 1, 2], j % 3)]
        m = b.molecule(p, rng.integers(0, 4, 3), rotate=False)
        b.bond(m, 0, 1), b.bond(m, 1, 2)
        b.angle(m, 0, 1, 2, k0=rng.uniform(20, 60), th0=pi if j % 2 == 0 else 2.5)
        special.append(("linear", m))
    s = b.build("edges", _size(size, 2000, 6000), 7.0, straddle_wrap=False, check=False)
    # ions paired by bonds: four longer than the cutoff as they are, and ten moved to (start, start + (cutoff + k ulps)
    # along a random direction clear of other atoms), positions exactly representable in `dtype` so that the oracle on
    # the rounded inputs sees the same distances
    inv_perm = np.argsort(s.meta["perm"])  # old index of each new atom
    nmolat = sum(len(m["pos"]) for m in b.mols)
    ions = list(rng.permutation(np.flatnonzero(inv_perm >= nmolat)))
    pos = s.pos.copy()
    L = s.box[0]
    wrapped = pos - np.floor(pos / L) * L

    def min_dist(x, skip):
        d = wrapped - (x - np.floor(x / L) * L)
        d -= L * np.round(d / L)
        r = np.linalg.norm(d, axis=1)
        r[skip] = np.inf
        return r.min()

    long_pairs = []
    while len(long_pairs) < 4:
        a = ions.pop()
        d = wrapped[ions] - wrapped[a]
        d -= L * np.round(d / L)
        r = np.linalg.norm(d, axis=1)
        c = [ions[k] for k in np.flatnonzero((r > cutoff + 0.3) & (r < cutoff + 4))][:1]
        if c:
            ions.remove(c[0])
            long_pairs.append((a, c[0]))
    offsets = [-2, -1, 0, 1, 2] * 2
    npdt = np.float32 if dtype == torch.float32 else np.float64
    near_pairs = []
    for k in offsets:
        a, c = ions.pop(), ions.pop()
        start = np.asarray(pos[a], dtype=npdt).astype(np.float64)
        while True:
            d = rng.standard_normal(3)
            d /= np.linalg.norm(d)
            far = near_cutoff_positions(dtype, cutoff, start, d, offsets=(k,))[0]
            if min_dist(far, [a, c]) > 2.5:
                break
        pos[a], pos[c] = start, far
        wrapped[c] = far - np.floor(far / L) * L
        near_pairs.append((a, c))
    g = dict(s.g)
    nb, npb = len(g["par_bond_idx"]), len(g["par_bond_params"])
    pairs = np.array(long_pairs + near_pairs, dtype=np.int64)
    r_long = [np.linalg.norm((lambda d: d - L * np.round(d / L))(pos[a] - pos[c])) for a, c in long_pairs]
    prm = np.concatenate([np.stack([np.full(4, 20.0), np.array(r_long) + rng.uniform(-0.05, 0.05, 4)], 1),
                          np.stack([rng.uniform(0.5, 2.0, len(near_pairs)), np.full(len(near_pairs), cutoff - 1.0)], 1)])
    g["par_bond_idx"] = np.concatenate([g["par_bond_idx"], pairs])
    g["par_bond_map"] = np.concatenate([g["par_bond_map"], np.stack([nb + np.arange(len(pairs)), npb + np.arange(len(pairs))], 1)])
    g["par_bond_params"] = np.concatenate([g["par_bond_params"], prm])
    meta = dict(s.meta)
    meta["long_bonds"] = nb + np.arange(4)
    meta["near_cutoff_bonds"] = nb + 4 + np.arange(len(near_pairs))
    meta["near_cutoff_offsets"] = np.array(offsets)
    # rows of the special angles / bonds in the permuted tables
    perm = s.meta["perm"]
    base = {}
    acc = 0
    for m in b.mols:
        base[id(m)] = acc
        acc += len(m["pos"])

    def rows_of(kind, mols, width):
        idx = g[f"par_{kind}_idx"]
        want = {tuple(perm[base[id(m)] + np.arange(len(m["pos"]))][list(t[:width])]) for m in mols for t in m[kind + "s"]}
        return np.array([r for r in range(len(idx)) if tuple(idx[r]) in want], dtype=np.int64)

    meta["near_linear_angles"] = rows_of("angle", [m for k, m in special if k == "near_linear"], 3)
    meta["linear_angles"] = rows_of("angle", [m for k, m in special if k == "linear"], 3)
    s = System(f"edges-{'f32' if dtype == torch.float32 else 'f64'}", g, pos, s.box, meta)
    assert len(meta["near_linear_angles"]) == 8 and len(meta["linear_angles"]) == 4 and len(meta["long_bonds"]) == 4
    s.meta["linear_angles_all"] = np.concatenate([meta["linear_angles"], meta["near_linear_angles"]])
    _check_geometry(System(s.name, g, pos, s.box, dict(meta, linear_angles=s.meta["linear_angles_all"])))
    _assert_light(s)
    return s


BUILDERS = {"light-full": light_full, "light-plus-one": light_plus_one, "hub": hub, "harmonic": harmonic,
            "harmonic-dihedrals": harmonic_dihedrals}


def build(name, size=SMALL, dtype=torch.float64):
    if name == "edges":
        return edges(dtype, size)
    return BUILDERS[name](size)


def positions_for(s, R, dtype, seed=0, jitter=0.02):
    """[R, N, 3] positions and [R, 3, 3] boxes: replica 0 is the system itself, replica r > 0 has its box scaled by
    (1 + 0.01 r) (coordinates scaled with it, so that every bond keeps its image) and the positions displaced."""
    rng = np.random.default_rng(seed)
    pos, box = [], []
    for r in range(R):
        sc = 1.0 + 0.01 * r
        pos.append(s.pos * sc + (jitter * rng.standard_normal(s.pos.shape) if r else 0.0))
        box.append(s.box * sc)
    pos = torch.tensor(np.stack(pos)).to(dtype)
    b = torch.zeros(R, 3, 3, dtype=dtype)
    for r in range(R):
        b[r].diagonal().copy_(torch.tensor(box[r]))
    return pos, b
