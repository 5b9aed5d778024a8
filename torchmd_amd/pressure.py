"""The instantaneous pressure from the molecular virial: host-side tables and unit handling.

    P_aa V = sum_I M_I V_I,a^2 + W_aa        P = (P_xx + P_yy + P_zz) / 3

with the sums over molecules I (mass M_I, centre-of-mass velocity V_I) and W the virial of the nonbonded force field under a
rigid displacement of whole molecules, evaluated on the GPU by `tmdhip_pressure` (csrc/virial.hip).  Molecules are the
connected components of the bond graph (`wrapper.calculate_molecule_groups`, the barostat's definition); an atom without
bonds is a molecule of one, a virtual site belongs to the molecule of its parents.  Bonded terms, constraint forces and
every other force inside a molecule do no work under such a displacement and never enter; for that to hold every exclusion
and every site's parents must lie inside one molecule, which `check_molecules` verifies once.

The pressure is that of the force field: `external` forces, restraints and the metadynamics bias are not part of it, and
there is no long-range dispersion correction (as in the energy).  Public entry points: `Forces.virial`,
`Integrator.pressure`, `Integrator.pressure_tensor`.
"""

from __future__ import annotations

import numpy as np

from .barostat import BAR_TO_KCAL_MOL_A3
from .wrapper import calculate_molecule_groups

__all__ = ["molecule_table", "check_molecules", "check_edges", "to_bar", "BAR_TO_KCAL_MOL_A3"]


def molecule_table(natoms, bonds, virtual_sites=None):
    """(offsets [nmol + 1], members [natoms], mol_of [natoms]), int32: the connected components of the bond graph, with
    every virtual site joined to its first parent."""
    edges = [np.asarray(bonds, dtype=np.int64).reshape(-1, 2)] if bonds is not None and len(bonds) else []
    if virtual_sites is not None and virtual_sites.nsites:
        edges.append(np.stack([np.asarray(virtual_sites.sites, dtype=np.int64), np.asarray(virtual_sites.parents, dtype=np.int64)[:, 0]], axis=1))
    off, mem = calculate_molecule_groups(natoms, np.concatenate(edges) if edges else None)
    off = np.ascontiguousarray(off, dtype=np.int32)
    mem = np.ascontiguousarray(mem, dtype=np.int32)
    mol_of = np.empty(natoms, dtype=np.int32)
    mol_of[mem] = np.repeat(np.arange(len(off) - 1, dtype=np.int32), np.diff(off))
    return off, mem, mol_of


def check_molecules(mol_of, excl_csr, virtual_sites=None):
    """ValueError when an excluded pair, or a virtual site and one of its parents, lie in two molecules: the force between
    them would then be intermolecular, and the molecular virial leaves it out."""
    off, idx = excl_csr
    rows = np.repeat(np.arange(len(off) - 1), np.diff(off))
    bad = np.nonzero(mol_of[rows] != mol_of[np.asarray(idx, dtype=np.int64)])[0] if len(idx) else []
    if len(bad):
        raise ValueError(f"pressure: the excluded pair ({rows[bad[0]]}, {idx[bad[0]]}) spans two molecules; the molecular virial "
                         "needs every exclusion inside one molecule (connected component of the bond graph)")
    if virtual_sites is not None and virtual_sites.nsites:
        sites = np.asarray(virtual_sites.sites, dtype=np.int64)
        parents = np.asarray(virtual_sites.parents, dtype=np.int64)
        for col in range(parents.shape[1]):
            used = parents[:, col] >= 0
            wrong = np.nonzero(used & (mol_of[np.where(used, parents[:, col], 0)] != mol_of[sites]))[0]
            if len(wrong):
                raise ValueError(f"pressure: the parents of virtual site {sites[wrong[0]]} lie in two molecules")


def check_edges(edges):
    if not (np.asarray(edges) > 0).all():
        raise ValueError("a pressure needs a periodic box: every box edge must be positive")


def to_bar(x):
    """kcal/mol/A^3 -> bar."""
    return np.asarray(x, dtype=np.float64) / BAR_TO_KCAL_MOL_A3
