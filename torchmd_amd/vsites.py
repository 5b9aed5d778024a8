"""Virtual interaction sites: massless sites whose position is a fixed linear combination of their parents'.

`VirtualSites(sites, parents, weights)` describes linear sites, r_site = sum_k w_k r_parent_k with two or three parents and
sum_k w_k = 1 (OpenMM's TwoParticleAverage / ThreeParticleAverage).  That covers the charge site of the whole TIP4P family
(TIP4P-Ew, TIP4P/2005) and of OPC.  A site carries charge and/or LJ parameters like any atom but has no mass: it is placed
before every force evaluation and hands the force it received to its parents afterwards (F_parent_k += w_k F_site), which
is exact for a linear site — total force and total torque are unchanged.

Out of scope: out-of-plane sites (TIP5P's lone pairs need a cross product of the parents' bond vectors) and sites built
from other sites.  Both are refused.

`construct` and `spread` are the numpy reference of the device kernels (csrc/vsite.hip) and serve the host-side start-up
path of the integrator; `Forces(..., virtual_sites=vs)` and `Integrator` use the kernels.
"""

from __future__ import annotations

import numpy as np

WEIGHT_SUM_TOLERANCE = 1e-12


class VirtualSites:
    """sites [S] atom indices; parents [S, 2 or 3] atom indices (-1 in the third column: a two-parent site);
    weights [S, 2 or 3] float64.  `masses` ([N], optional) lets the constructor check what only the topology knows: a site
    has mass 0, a parent has not."""

    def __init__(self, sites, parents, weights, masses=None):
        s = np.asarray(sites, dtype=np.int64).reshape(-1)
        p = np.asarray(parents, dtype=np.int64)
        w = np.asarray(weights, dtype=np.float64)
        if p.ndim != 2 or p.shape[0] != len(s) or p.shape[1] not in (2, 3) or w.shape != p.shape:
            raise ValueError("virtual sites: parents and weights must be [nsites, 2] or [nsites, 3]")
        if p.shape[1] == 2:
            p = np.concatenate([p, -np.ones((len(s), 1), dtype=np.int64)], axis=1)
            w = np.concatenate([w, np.zeros((len(s), 1))], axis=1)
        unused = p[:, 2] < 0
        w = np.where(np.stack([np.zeros_like(unused), np.zeros_like(unused), unused], axis=1), 0.0, w)
        if len(s) and ((s < 0).any() or (p[:, :2] < 0).any() or (p < -1).any()):
            raise ValueError("virtual sites: negative atom index")
        if not np.isfinite(w).all():
            raise ValueError("virtual sites: weights must be finite")
        if len(s) and np.abs(w.sum(axis=1) - 1.0).max() > WEIGHT_SUM_TOLERANCE:
            raise ValueError("virtual sites: the weights of a site must sum to 1 (within 1e-12)")
        if len(np.unique(s)) != len(s):
            raise ValueError("virtual sites: a site is listed twice")
        used = p[p >= 0]
        for k in range(len(s)):
            row = p[k][p[k] >= 0]
            if len(np.unique(row)) != len(row):
                raise ValueError(f"virtual sites: site {s[k]} lists a parent twice")
        if np.isin(used, s).any():
            raise ValueError("virtual sites: a site cannot be its own parent or a parent of another site "
                             "(sites built from sites are not supported)")
        if len(np.unique(used)) != len(used):
            raise ValueError("virtual sites: two sites share a parent (the force spreading writes every parent once, "
                             "without atomics)")
        self.sites = np.ascontiguousarray(s, dtype=np.int32)
        self.parents = np.ascontiguousarray(p, dtype=np.int32)
        self.weights = np.ascontiguousarray(w, dtype=np.float64)
        if masses is not None:
            self.check_masses(masses)

    def __len__(self):
        return len(self.sites)

    @property
    def nsites(self):
        return len(self.sites)

    def check_masses(self, masses):
        """A site has no mass, a parent has one.  `masses` [N] or [N, 1]."""
        m = np.asarray(masses.detach().cpu().numpy() if hasattr(masses, "detach") else masses, dtype=np.float64).reshape(-1)
        if len(self.sites) and (self.sites.max() >= len(m) or self.parents.max() >= len(m)):
            raise ValueError("virtual sites: atom index out of range")
        if (m[self.sites] != 0).any():
            raise ValueError("virtual sites: a site must have mass 0")
        used = self.parents[self.parents >= 0]
        if (m[used] <= 0).any():
            raise ValueError("virtual sites: a parent must have a mass (> 0)")

    def site_mask(self, natoms):
        mask = np.zeros(int(natoms), dtype=bool)
        mask[self.sites] = True
        return mask

    def exclusion_pairs(self):
        """Every (site, parent) pair, [K, 2] int64: a site never interacts with the atoms it is built from."""
        k = self.parents >= 0
        return np.stack([np.repeat(self.sites.astype(np.int64), k.sum(axis=1)), self.parents[k].astype(np.int64)], axis=1)

    @classmethod
    def tip4p(cls, topology_or_nmol, r_om, r_oh, theta, masses=None):
        """The M site of nmol four-site waters in atom order O, H1, H2, M: on the H-O-H bisector at `r_om` from the oxygen,
        a = r_OM / (2 r_OH cos(theta / 2)), weights (1 - 2a, a, a).  `theta` in degrees.  `topology_or_nmol`: the molecule
        count, or a topology (`numAtoms`, a multiple of 4)."""
        if hasattr(topology_or_nmol, "numAtoms"):
            natoms = int(topology_or_nmol.numAtoms)
            if natoms % 4:
                raise ValueError("VirtualSites.tip4p: the topology must hold four-site molecules only (O, H1, H2, M)")
            nmol = natoms // 4
            if masses is None and getattr(topology_or_nmol, "masses", None) is not None:
                masses = topology_or_nmol.masses
        else:
            nmol = int(topology_or_nmol)
        a = float(r_om) / (2.0 * float(r_oh) * np.cos(0.5 * np.deg2rad(float(theta))))
        base = 4 * np.arange(nmol, dtype=np.int64)
        parents = np.stack([base, base + 1, base + 2], axis=1)
        weights = np.tile(np.array([1.0 - 2.0 * a, a, a]), (nmol, 1))
        return cls(base + 3, parents, weights, masses=masses)

    # ------------------------------------------------------------------ numpy reference of csrc/vsite.hip
    def construct(self, pos):
        """Place the sites: pos [..., N, 3] in place (and returned); parents summed in table order, in float64."""
        x = np.asarray(pos)
        p, w = self.parents, self.weights
        acc = w[:, 0, None] * x[..., p[:, 0], :].astype(np.float64)
        acc = acc + w[:, 1, None] * x[..., p[:, 1], :].astype(np.float64)
        three = p[:, 2] >= 0
        third = w[:, 2, None] * x[..., np.where(three, p[:, 2], 0), :].astype(np.float64)
        acc = np.where(three[:, None], acc + third, acc)
        x[..., self.sites, :] = acc.astype(x.dtype)
        return x

    def spread(self, forces):
        """Hand every site's force to its parents: forces [..., N, 3] in place (and returned);
        F_parent_k += w_k F_site in float64, then F_site = 0."""
        f = np.asarray(forces)
        fs = f[..., self.sites, :].astype(np.float64)
        for k in range(3):
            sel = self.parents[:, k] >= 0
            if not sel.any():
                continue
            idx = self.parents[sel, k]
            f[..., idx, :] = (f[..., idx, :].astype(np.float64) + self.weights[sel, k, None] * fs[..., sel, :]).astype(f.dtype)
        f[..., self.sites, :] = 0
        return f
