"""Holonomic constraints: topology analysis (host, numpy) for rigid waters and X-H bonds.

`find_constraints(masses, bond_params, angle_params, mode)` turns the bond table of a `Parameters` object into the two kinds
of units the constrained MD step integrates (include/tmdhip.h, tmdhip_set_constraints):

* rigid waters — three atoms, one heavy atom bonded to two hydrogens and nothing else; solved by analytic SETTLE
  (Miyamoto & Kollman 1992).  d_OH comes from the O-H bond's `req`, d_HH from the H-H bond's `req`, or from d_OH and the
  H-O-H angle's theta0 when the H-H bond is missing;
* X-H clusters ("hbonds" only) — a heavy atom and the hydrogens bonded to it (1 .. 4 bonds), central atom first; solved by
  iterated SHAKE.

A hydrogen is an atom of mass < 1.5 amu.  `ConstraintSet.ndof()` counts the degrees of freedom the reported temperature
divides by: 3 N minus the number of constraints (a rigid water counts 3), the centre-of-mass motion not subtracted.

Virtual sites (`vsites.VirtualSites`) are no atoms here: a massless site is never a hydrogen, every bond or angle
that touches one is ignored, and a site adds no degrees of freedom (ndof = 3 (N - N_sites) - N_constraints).  Every site's
parents must be the three atoms of one rigid water, the heavy atom first: the water's thread of the constrained MD step
carries the site (`ConstraintSet.water_sites`).

The start-up projection of `Integrator` (`shake_positions`, `project_velocities`) is vectorised over the units: constraint
slot k of every unit at once (the units touch disjoint atoms), Gauss-Seidel over the slots.
"""

from __future__ import annotations

import numpy as np

HYDROGEN_MASS = 1.5  # amu: lighter atoms are hydrogens
MODES = ("water", "hbonds")
MAX_CLUSTER_BONDS = 4
SHAKE_TOLERANCE = 1e-10  # relative bond-length tolerance of the device SHAKE
SHAKE_MAX_ITER = 200


def _table(tab, width):
    if tab is None:
        return np.zeros((0, width), dtype=np.int64), np.zeros(0)
    idx = np.asarray(_host(tab["idx"]), dtype=np.int64).reshape(-1, width)
    mp = np.asarray(_host(tab["map"]), dtype=np.int64).reshape(-1, 2)
    prm = np.asarray(_host(tab["params"]), dtype=np.float64)
    return idx, prm[mp[:, 1]]


def _host(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


class ConstraintSet:
    """The constraints of one topology.

    waters      int32 [W, 3]   O, H1, H2
    water_dist  float64 [W, 2] d_OH, d_HH (Angstrom)
    offsets     int32 [C + 1]  CSR of the clusters into `atoms`
    atoms       int32          central atom first, then its hydrogens
    dist        float64        per entry of `atoms`: the bond length to the central atom (0 for the central atom)
    """

    def __init__(self, natoms, masses, waters, water_dist, offsets, atoms, dist, mode, nsites=0, water_sites=None):
        self.nsites = int(nsites)  # massless virtual sites among the atoms: no degrees of freedom
        self.water_sites = water_sites  # int32 [W]: the site each water carries, -1 = none (None: no sites at all)
        self.natoms = int(natoms)
        self.masses = np.asarray(masses, dtype=np.float64)
        self.waters = np.ascontiguousarray(waters, dtype=np.int32).reshape(-1, 3)
        self.water_dist = np.ascontiguousarray(water_dist, dtype=np.float64).reshape(-1, 2)
        self.offsets = np.ascontiguousarray(offsets, dtype=np.int32)
        self.atoms = np.ascontiguousarray(atoms, dtype=np.int32)
        self.dist = np.ascontiguousarray(dist, dtype=np.float64)
        self.mode = mode
        self.tolerance = SHAKE_TOLERANCE
        self.max_iter = SHAKE_MAX_ITER

    @property
    def nwaters(self):
        return len(self.waters)

    @property
    def nclusters(self):
        return len(self.offsets) - 1

    @property
    def nconstraints(self):
        return 3 * self.nwaters + len(self.atoms) - self.nclusters

    def clusters(self):
        return [self.atoms[self.offsets[c]:self.offsets[c + 1]] for c in range(self.nclusters)]

    def pairs(self):
        """Every constraint as (i, j, d): [K, 2] int64, [K] float64."""
        ij, d = [], []
        for (o, h1, h2), (doh, dhh) in zip(self.waters, self.water_dist):
            ij += [(o, h1), (o, h2), (h1, h2)]
            d += [doh, doh, dhh]
        for c in range(self.nclusters):
            s, e = self.offsets[c], self.offsets[c + 1]
            for k in range(s + 1, e):
                ij.append((self.atoms[s], self.atoms[k]))
                d.append(self.dist[k])
        return np.asarray(ij, dtype=np.int64).reshape(-1, 2), np.asarray(d, dtype=np.float64)

    def ndof(self, batch=None):
        """3 N - N_constraints, per atom group when `batch` (natoms,) assigns atoms to groups."""
        if batch is None:
            return 3 * (self.natoms - self.nsites) - self.nconstraints
        b = np.asarray(_host(batch), dtype=np.int64)
        ng = int(b.max()) + 1
        dof = 3 * np.bincount(b, weights=(self.masses > 0) if self.nsites else None, minlength=ng).astype(np.int64)
        ij, _ = self.pairs()
        if len(ij):
            if np.any(b[ij[:, 0]] != b[ij[:, 1]]):
                raise ValueError("constraints: a constrained bond joins two atom groups of `batch`")
            dof -= np.bincount(b[ij[:, 0]], minlength=ng)
        return dof

    # -------------------------------------------------------------- start-up projection (fp64, vectorised)
    def _slots(self):
        """Constraint slot k of every unit: (i, j, d) arrays, units disjoint within a slot."""
        if getattr(self, "_slot_cache", None) is None:
            slots = []
            w, wd = self.waters.astype(np.int64), self.water_dist
            if len(w):
                slots += [(w[:, 0], w[:, 1], wd[:, 0]), (w[:, 0], w[:, 2], wd[:, 0]), (w[:, 1], w[:, 2], wd[:, 1])]
            off = self.offsets.astype(np.int64)
            size = np.diff(off)
            for k in range(1, MAX_CLUSTER_BONDS + 1):
                sel = np.nonzero(size > k)[0]
                if len(sel):
                    slots.append((self.atoms[off[sel]].astype(np.int64), self.atoms[off[sel] + k].astype(np.int64),
                                  self.dist[off[sel] + k]))
            self._slot_cache = slots
        return self._slot_cache

    def _inverse_masses(self):
        # (massless virtual sites are in no constraint: their entry is never read)
        return np.divide(1.0, self.masses, out=np.zeros_like(self.masses), where=self.masses > 0)

    def shake_positions(self, x, ref, tol=1e-13, max_iter=1000):
        """SHAKE `x` [N, 3] (fp64, in place) onto the constraints along the bond vectors of `ref`."""
        im = self._inverse_masses()
        slots = self._slots()
        for _ in range(max_iter):
            worst = 0.0
            for i, j, d in slots:
                s = x[i] - x[j]
                diff = d * d - np.einsum("ij,ij->i", s, s)
                worst = max(worst, float(np.max(np.abs(diff) / (d * d))) if len(d) else 0.0)
                r = ref[i] - ref[j]
                g = diff / (2.0 * np.einsum("ij,ij->i", r, s) * (im[i] + im[j]))
                x[i] += (g * im[i])[:, None] * r
                x[j] -= (g * im[j])[:, None] * r
            if worst < 2 * tol:
                return x
        raise RuntimeError("constraints: the start-up SHAKE did not converge (positions too far from the constrained geometry)")

    def project_velocities(self, x, v, sweeps=200, tol=1e-14):
        """Remove the velocity components along every constraint (v [N, 3] fp64, in place), Gauss-Seidel over the slots."""
        im = self._inverse_masses()
        slots = self._slots()
        for _ in range(sweeps):
            worst = 0.0
            for i, j, _d in slots:
                r = x[i] - x[j]
                rv = np.einsum("ij,ij->i", r, v[i] - v[j])
                rr = np.einsum("ij,ij->i", r, r)
                mu = -rv / (rr * (im[i] + im[j]))
                v[i] += (mu * im[i])[:, None] * r
                v[j] -= (mu * im[j])[:, None] * r
                if len(rv):
                    worst = max(worst, float(np.max(np.abs(rv) / np.sqrt(rr))))
            if worst < tol:
                break
        return v


def find_constraints(masses, bond_params, angle_params=None, mode="water", virtual_sites=None):
    """Rigid waters (and, with mode="hbonds", X-H clusters) of a topology.  `masses` [N] or [N, 1]; `bond_params` /
    `angle_params`: the `Parameters` tables ({"idx", "map", "params"}; params[:, 1] = req / theta0).  `virtual_sites`: a
    `vsites.VirtualSites` — the sites, and every bond or angle that touches one, are left out of the search; every site's
    parents must then be the atoms of one rigid water (heavy atom first), whose hydrogens are listed in the parents' order."""
    if mode not in MODES:
        raise ValueError(f"constraints must be None, 'water' or 'hbonds', got {mode!r}")
    m = np.asarray(_host(masses), dtype=np.float64).reshape(-1)
    n = len(m)
    is_site = np.zeros(n, dtype=bool)
    if virtual_sites is not None and virtual_sites.nsites:
        virtual_sites.check_masses(m)
        is_site = virtual_sites.site_mask(n)
    hyd = (m < HYDROGEN_MASS) & ~is_site
    bidx, bprm = _table(bond_params, 2)
    breq = bprm[:, 1] if len(bprm) else np.zeros(0)
    keep = (bidx[:, 0] != bidx[:, 1]) & ~is_site[bidx[:, 0]] & ~is_site[bidx[:, 1]]
    if len(breq) == len(bidx):
        breq = breq[keep]
    bidx = bidx[keep]
    breq = breq[: len(bidx)] if len(breq) == len(bidx) else breq
    neigh = [dict() for _ in range(n)]  # atom -> {bonded atom: req}
    for (i, j), r in zip(bidx, breq):
        neigh[i][j] = float(r)
        neigh[j][i] = float(r)
    aidx, aprm = _table(angle_params, 3)
    theta = {}
    for (i, j, k), p in zip(aidx, aprm):
        if is_site[i] or is_site[j] or is_site[k]:
            continue
        theta[(int(i), int(j), int(k))] = theta[(int(k), int(j), int(i))] = float(p[1])

    # rigid waters: a heavy atom bonded to exactly two hydrogens, which are bonded to nothing but it and each other
    in_water = np.zeros(n, dtype=bool)
    waters, wdist = [], []
    for o in range(n):
        if hyd[o] or is_site[o]:
            continue
        nb = list(neigh[o])
        if len(nb) != 2 or not (hyd[nb[0]] and hyd[nb[1]]):
            continue
        h1, h2 = sorted(nb)
        if set(neigh[h1]) - {o, h2} or set(neigh[h2]) - {o, h1}:
            continue
        d1, d2 = neigh[o][h1], neigh[o][h2]
        if abs(d1 - d2) > 1e-6 * d1 or m[h1] != m[h2]:
            raise ValueError(f"constraints: water {o} has unequal O-H bonds or hydrogen masses (SETTLE needs a symmetric molecule)")
        if h2 in neigh[h1]:
            dhh = neigh[h1][h2]
        elif (h1, o, h2) in theta:
            dhh = 2.0 * d1 * np.sin(0.5 * theta[(h1, o, h2)])
        else:
            raise ValueError(f"constraints: water {o} has neither an H-H bond nor an H-O-H angle")
        waters.append((o, h1, h2))
        wdist.append((d1, dhh))
        in_water[[o, h1, h2]] = True

    offsets, atoms, dist = [0], [], []
    if mode == "hbonds":
        owner = -np.ones(n, dtype=np.int64)
        cl = {}
        for i in range(n):
            if not hyd[i] or in_water[i]:
                continue
            heavy = [j for j in neigh[i] if not hyd[j]]
            if len(heavy) > 1:
                raise ValueError(f"constraints: hydrogen {i} is in two constraints outside a water (bonded to {heavy})")
            if not heavy:
                continue
            owner[i] = heavy[0]
            cl.setdefault(heavy[0], []).append(i)
        for x in sorted(cl):
            hs = sorted(cl[x])
            if len(hs) > MAX_CLUSTER_BONDS:
                raise ValueError(f"constraints: a cluster of {len(hs)} constraints around atom {x} (at most {MAX_CLUSTER_BONDS})")
            atoms += [x] + hs
            dist += [0.0] + [neigh[x][h] for h in hs]
            offsets.append(len(atoms))
    nsites, water_sites = 0, None
    if is_site.any():
        # every site rides with the rigid water its parents form
        nsites = int(is_site.sum())
        water_of = {int(w[0]): k for k, w in enumerate(waters)}
        water_sites = -np.ones(len(waters), dtype=np.int32)
        waters = [list(w) for w in waters]
        for s, pa in zip(virtual_sites.sites, virtual_sites.parents):
            k = water_of.get(int(pa[0]))
            if k is None or pa[2] < 0 or {int(pa[1]), int(pa[2])} != {int(waters[k][1]), int(waters[k][2])} or water_sites[k] >= 0:
                raise ValueError(f"constraints: the parents of virtual site {int(s)} must be exactly the three atoms of one rigid "
                                 "water, the heavy atom first (sites on flexible molecules are supported by Forces.compute only)")
            waters[k][1], waters[k][2] = int(pa[1]), int(pa[2])  # (SETTLE is symmetric in the hydrogens)
            water_sites[k] = int(s)
    return ConstraintSet(n, m, np.asarray(waters, dtype=np.int32).reshape(-1, 3), np.asarray(wdist).reshape(-1, 2),
                         np.asarray(offsets), np.asarray(atoms, dtype=np.int32), np.asarray(dist, dtype=np.float64), mode,
                         nsites=nsites, water_sites=water_sites)
