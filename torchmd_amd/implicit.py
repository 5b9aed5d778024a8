"""Generalized-Born implicit solvent: OBC2 (Onufriev, Bashford, Case 2004) with the ACE-type surface-area term.

    gb = GeneralizedBorn.from_parameters(parameters)          # or GeneralizedBorn(radii, scale, ...)
    forces = Forces(parameters, terms=..., implicit_solvent=gb)

For systems with open boundaries (box [0, 0, 0]) that carry no water.  `compute()` adds the force, reports an
"implicit_solvent" entry (GB + SA) that is part of the total, `minimize_fire` converges on the total and `Integrator.step`
integrates under the total force and returns the total potential energy.  The GB sums run over every pair of atoms: they never
use the cutoff of the vacuum terms, no exclusions and no minimum image."""

from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L

# The defaults of `GeneralizedBorn.from_parameters`: the helper's own table by element, not a named published set.
DEFAULT_RADII = {"H": 1.2, "C": 1.7, "N": 1.55, "O": 1.5, "F": 1.5, "P": 1.85, "S": 1.8, "Cl": 1.7}
RADIUS_H_ON_N = 1.3
RADIUS_OTHER = 1.5
DEFAULT_SCALES = {"H": 0.85, "C": 0.72, "N": 0.79, "O": 0.85, "F": 0.88, "P": 0.86, "S": 0.96}
SCALE_OTHER = 0.8
_ELEMENT_BY_MASS = {1: "H", 12: "C", 14: "N", 16: "O", 19: "F", 31: "P", 32: "S", 35: "Cl"}
OFFSET = 0.09


def elements_from_masses(masses):
    """Masses rounded to whole numbers -> element symbols (None where the table has none)."""
    m = np.asarray(masses, dtype=np.float64).reshape(-1)
    return [_ELEMENT_BY_MASS.get(int(round(float(x)))) for x in m]


class GeneralizedBorn(L.SideTerm):
    """Per-atom intrinsic radii (A) and descreening scales, the two dielectric constants, the surface tension (kcal/mol/A^2;
    0 switches the surface-area term off) and the probe radius (A).  ValueError: a radius <= 0.09 or not finite, a negative
    scale, a dielectric constant <= 0, arrays of different lengths."""

    side_name, side_width = "implicit_solvent", 2  # (GB, SA)
    side_apply, side_energy = "tmdhip_gb_apply", "tmdhip_gb_energy"
    refusals = {
        "vmap": "compute() with implicit_solvent cannot run under torch.vmap (its Born radii are per replica of the context)",
        "batch": "implicit_solvent does not support atom groups (batch=): its Born radii are per replica",
        "barostat": "implicit_solvent cannot run under barostat=: open boundaries have no volume",
        "update_atoms": "update_atoms is not available with implicit_solvent",
        "pressure": "the pressure and the virial are not available with implicit_solvent (open boundaries: there is no volume)",
        "domain": "implicit_solvent cannot be domain-decomposed (the generalized-Born sums run over all pairs of atoms, "
                  "and a brick holds passive atoms)",
    }

    def __init__(self, radii, scale, solute_dielectric=1.0, solvent_dielectric=78.5, surface_tension=0.0054, probe_radius=1.4):
        self.radii = np.ascontiguousarray(np.asarray(radii, dtype=np.float64).reshape(-1))
        self.scale = np.ascontiguousarray(np.asarray(scale, dtype=np.float64).reshape(-1))
        if len(self.radii) != len(self.scale) or len(self.radii) == 0:
            raise ValueError("GeneralizedBorn: radii and scale must hold one entry per atom each")
        if not (np.isfinite(self.radii).all() and (self.radii > OFFSET).all()):
            raise ValueError("GeneralizedBorn: every radius must be finite and above 0.09 A")
        if not (np.isfinite(self.scale).all() and (self.scale >= 0).all()):
            raise ValueError("GeneralizedBorn: every scale must be finite and not negative")
        self.solute_dielectric = float(solute_dielectric)
        self.solvent_dielectric = float(solvent_dielectric)
        if not (np.isfinite([self.solute_dielectric, self.solvent_dielectric]).all() and self.solute_dielectric > 0
                and self.solvent_dielectric > 0):
            raise ValueError("GeneralizedBorn: the dielectric constants must be finite and positive")
        self.surface_tension = float(surface_tension)
        self.probe_radius = float(probe_radius)
        if not (np.isfinite([self.surface_tension, self.probe_radius]).all() and self.surface_tension >= 0 and self.probe_radius >= 0):
            raise ValueError("GeneralizedBorn: the surface tension and the probe radius must be finite and not negative")
        self.energy = None  # [R, 2] (GB, SA) of the last synchronous evaluation, host

    @property
    def natoms(self):
        return len(self.radii)

    @classmethod
    def from_parameters(cls, parameters, **kw):
        """Default radii and scales from the masses (rounded to elements) and the bond table of `parameters`: a hydrogen
        counts as bonded to nitrogen when `bond_params["idx"]` says so.
        Radii: H 1.2, H on N 1.3, C 1.7, N 1.55, O 1.5, F 1.5, P 1.85, S 1.8, Cl 1.7, otherwise 1.5.
        Scales: H 0.85, C 0.72, N 0.79, O 0.85, F 0.88, P 0.86, S 0.96, otherwise 0.8.
        These are this helper's defaults, not a named published set: pass arrays of your own to the constructor otherwise."""
        import torch

        el = elements_from_masses(torch.as_tensor(parameters.masses).detach().cpu().double().reshape(-1).numpy())
        radii = np.array([DEFAULT_RADII.get(e, RADIUS_OTHER) for e in el], dtype=np.float64)
        scale = np.array([DEFAULT_SCALES.get(e, SCALE_OTHER) for e in el], dtype=np.float64)
        bp = getattr(parameters, "bond_params", None)
        if bp is not None and bp.get("idx") is not None and len(bp["idx"]):
            for a, b in torch.as_tensor(bp["idx"]).detach().cpu().numpy().reshape(-1, 2):
                for h, x in ((a, b), (b, a)):
                    if el[h] == "H" and el[x] == "N":
                        radii[h] = RADIUS_H_ON_N
        return cls(radii, scale, **kw)

    def check(self, natoms):
        if self.natoms != natoms:
            raise ValueError(f"GeneralizedBorn: {self.natoms} radii and scales for {natoms} atoms")

    def upload(self, lib, ctx):
        d = L.GbDesc()
        d.struct_size = C.sizeof(L.GbDesc)
        d.enable = 1
        d.radii_host = self.radii.ctypes.data_as(C.c_void_p)
        d.scale_host = self.scale.ctypes.data_as(C.c_void_p)
        d.solute_dielectric, d.solvent_dielectric = self.solute_dielectric, self.solvent_dielectric
        d.surface_tension, d.probe_radius = self.surface_tension, self.probe_radius
        L.check(lib.tmdhip_set_gb(ctx, C.byref(d)), "tmdhip_set_gb")

    def sync(self, eng, owner=None):
        """Hand the model to the context of `eng` on first sight (tmdhip_set_gb)."""
        if eng.side_seen.get(self.side_name) is not self:
            self.upload(eng.lib, eng.ctx)
            eng.side_seen[self.side_name] = self
