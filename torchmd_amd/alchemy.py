"""Alchemical decoupling of a solute from its environment, one coupling per replica.

    al = Alchemical(atoms, lambda_vdw=[1.0, 0.5, 0.0], lambda_elec=[0.0, 0.0, 0.0], alpha=0.5)
    forces = Forces(parameters, terms=..., cutoff=9.0, rfa=True, alchemical=al)

Convention: decoupling.  The pairs between the solute S and every other atom are scaled: soft-core Lennard-Jones

    s = r^6 + alpha sigma^6 (1 - lambda_vdw),   U_lj = lambda_vdw (A / s^2 - B / s) sw(r),   sigma^6 = A / B

and lambda_elec times the context's electrostatics (no soft core on the charges: every replica needs lambda_elec = 0 or
lambda_vdw = 1).  The pairs inside S, its 1-4 terms and its bonded terms stay at full strength; everything else is untouched.
`compute()` reports an "alchemical" entry (cross + intra) inside the total, `Forces.alchemical_terms()` returns
(cross LJ, cross electrostatics, intra, dU/dlambda_vdw, dU/dlambda_elec) per replica for thermodynamic integration, and
`Forces.alchemical_energies(pos, box, states)` the cross energy at other couplings for BAR / MBAR."""

from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L

MAX_STATES = 32  # of one tmdhip_alchemical_states call; `Forces.alchemical_energies` serves more in several calls


def check_lambdas(vdw, elec, what="Alchemical"):
    """lambda in [0, 1], and the staging rule lambda_elec = 0 or lambda_vdw = 1 (ValueError otherwise)."""
    vdw, elec = np.asarray(vdw, dtype=np.float64), np.asarray(elec, dtype=np.float64)
    if not (np.all(np.isfinite(vdw)) and np.all(np.isfinite(elec)) and np.all((vdw >= 0) & (vdw <= 1)) and np.all((elec >= 0) & (elec <= 1))):
        raise ValueError(f"{what}: every lambda must lie in [0, 1]")
    if np.any((elec != 0) & (vdw != 1)):
        raise ValueError(f"{what}: the charges have no soft core, so lambda_elec must be 0 or lambda_vdw must be 1 "
                         "(switch the charges off before the spheres soften)")


def append_null_class(A, B, types, atoms):
    """The tables `tmdhip_create` gets with a solute: an all-zero Lennard-Jones class appended behind the (already merged)
    classes, and the solute's atoms moved into it.  The class is appended AFTER `merge_lj_types`, so that it never shares a row
    with another all-zero class whose atoms carry charge (TIP3P hydrogen): the fp32 kernel's charge-by-class path needs the
    charge to be a function of the class.  Returns (A2, B2, types2, the solute's true classes)."""
    A, B = np.asarray(A), np.asarray(B)
    types = np.asarray(types).astype(np.int64).copy()
    atoms = np.asarray(atoms, dtype=np.int64)
    T = A.shape[0]
    A2 = np.zeros((T + 1, T + 1), dtype=A.dtype)
    B2 = np.zeros((T + 1, T + 1), dtype=B.dtype)
    A2[:T, :T], B2[:T, :T] = A, B
    classes = types[atoms].astype(np.int32)
    types[atoms] = T
    return np.ascontiguousarray(A2), np.ascontiguousarray(B2), types, np.ascontiguousarray(classes)


def _tuples(tab, width):
    if tab is None or tab.get("idx") is None or len(tab["idx"]) == 0:
        return np.zeros((0, width), dtype=np.int32)
    idx = tab["idx"]
    idx = idx.detach().cpu().numpy() if hasattr(idx, "detach") else np.asarray(idx)
    return np.ascontiguousarray(idx.reshape(-1, width).astype(np.int32))


def check_closed(atoms, natoms, tuples):
    """ValueError unless every tuple of `tuples` ({name: [M, width] indices}) that names an atom of the solute names only
    atoms of the solute."""
    mask = np.zeros(natoms, dtype=bool)
    mask[np.asarray(atoms, dtype=np.int64)] = True
    for name, idx in tuples.items():
        if len(idx) == 0:
            continue
        inside = mask[np.asarray(idx, dtype=np.int64)].sum(axis=1)
        bad = np.nonzero((inside != 0) & (inside != idx.shape[1]))[0]
        if len(bad):
            raise ValueError(f"Alchemical: {name} {tuple(int(v) for v in idx[bad[0]])} joins the solute to the environment: the "
                             "solute must be closed under the topology")


class Alchemical(L.SideTerm):
    """`atoms`: the indices of the solute.  `lambda_vdw`, `lambda_elec`: scalars or one value per replica.  `alpha`: the
    soft-core parameter (>= 0).  ValueError: an index given twice or negative, a lambda outside [0, 1], a replica with
    lambda_elec != 0 and lambda_vdw != 1, alpha < 0."""

    side_name, side_width = "alchemical", 5  # (cross LJ, cross electrostatics, intra, dU/dlambda_vdw, dU/dlambda_elec)
    side_potential = slice(0, 3)  # cross + intra
    side_apply, side_energy = "tmdhip_alchemical_apply", "tmdhip_alchemical_energy"
    refusals = {
        "vmap": "compute() with alchemical= cannot run under torch.vmap (its couplings are per replica of the context)",
        "batch": "alchemical= does not support atom groups (batch=): its couplings are per replica",
        "barostat": "alchemical= cannot run under barostat=: the virial lacks the solute's term",
        "update_atoms": "update_atoms is not available with alchemical=",
        "pressure": "the pressure and the virial are not available with alchemical= (the virial lacks the solute's term)",
        "domain": "alchemical= cannot be domain-decomposed (the solute's atoms would straddle bricks, and atom indices "
                  "change at every migration)",
    }

    def __init__(self, atoms, lambda_vdw=1.0, lambda_elec=1.0, alpha=0.5):
        a = np.atleast_1d(np.asarray(atoms))
        if a.ndim != 1 or len(a) == 0 or not np.issubdtype(a.dtype, np.integer) or np.any(a < 0):
            raise ValueError("Alchemical: atoms must be a non-empty list of non-negative whole numbers")
        if len(np.unique(a)) != len(a):
            raise ValueError("Alchemical: an atom is given twice")
        self.atoms = np.ascontiguousarray(np.sort(a).astype(np.int32))
        self.alpha = float(alpha)
        if not (np.isfinite(self.alpha) and self.alpha >= 0):
            raise ValueError("Alchemical: alpha must be finite and not negative")
        self.version = 0
        self.set_lambdas(lambda_vdw, lambda_elec)
        self.energy = None  # [R, 5] of the last synchronous evaluation, host

    def set_lambdas(self, vdw, elec):
        """Move the couplings (scalars or one value per replica); the next evaluation uploads them."""
        v, e = np.atleast_1d(np.asarray(vdw, dtype=np.float64)), np.atleast_1d(np.asarray(elec, dtype=np.float64))
        if v.ndim != 1 or e.ndim != 1 or (len(v) != len(e) and 1 not in (len(v), len(e))):
            raise ValueError("Alchemical: lambda_vdw and lambda_elec must be scalars or hold one value per replica each")
        v, e = np.broadcast_arrays(v, e)
        check_lambdas(v, e)
        self.lambda_vdw, self.lambda_elec = v.copy(), e.copy()
        self.version += 1

    def lambdas(self, nreplicas):
        """([R], [R]) for a context of `nreplicas` replicas."""
        if len(self.lambda_vdw) not in (1, nreplicas):
            raise ValueError(f"Alchemical: {len(self.lambda_vdw)} couplings for {nreplicas} replicas")
        return (np.ascontiguousarray(np.broadcast_to(self.lambda_vdw, (nreplicas,)).astype(np.float64)),
                np.ascontiguousarray(np.broadcast_to(self.lambda_elec, (nreplicas,)).astype(np.float64)))

    # ------------------------------------------------------------------ exchange of couplings between replicas
    def exchange_parameters(self, nreplicas):
        """[R, 2] = (lambda_vdw, lambda_elec) per replica; None for one coupling shared by all replicas."""
        if len(self.lambda_vdw) == 1 and nreplicas != 1:
            return None
        return np.stack(self.lambdas(nreplicas), axis=1)

    def cross_energies(self, owner, pos, box, snapshot):
        """The cross energy at every state (the intra part is the same in all of them: a constant per row)."""
        return owner.alchemical_energies(pos, box, snapshot)

    def assign_states(self, snapshot, state_of_slot):
        s = np.asarray(snapshot)[np.asarray(state_of_slot, dtype=np.int64)]
        self.set_lambdas(s[:, 0], s[:, 1])

    def topology(self, parameters, energies):
        """The index tuples of the bonded terms that are on: {name: [M, width]}."""
        out = {}
        for name, attr, width in (("bond", "bond_params", 2), ("angle", "angle_params", 3), ("torsion", "dihedral_params", 4),
                                  ("improper", "improper_params", 4), ("1-4 pair", "nonbonded_14_params", 2)):
            term = {"bond": "bonds", "angle": "angles", "torsion": "dihedrals", "improper": "impropers", "1-4 pair": "1-4"}[name]
            out[name] = _tuples(getattr(parameters, attr, None), width) if term in energies else np.zeros((0, width), dtype=np.int32)
        return out

    def check(self, natoms, parameters, energies, excl_csr, tables=None):
        """What a `Forces` refuses (ValueError): an index beyond the system, a solute that is not closed under the topology
        (bonds, angles, torsions, 1-4 pairs, exclusions), the repulsion terms and, with `tables` = (A, B, types), a
        solute-environment pair with A > 0 >= B (sigma^6 = A / B does not exist) or A < 0."""
        if self.atoms[-1] >= natoms:
            raise ValueError(f"Alchemical: atom {int(self.atoms[-1])} is beyond the system's {natoms} atoms")
        if "repulsion" in energies or "repulsioncg" in energies:
            raise ValueError("alchemical= cannot be combined with the repulsion / repulsioncg terms")
        tuples = self.topology(parameters, energies)
        off, idx = excl_csr
        if len(idx):
            rows = np.repeat(np.arange(natoms), np.diff(np.asarray(off, dtype=np.int64)))
            tuples["exclusion"] = np.stack([rows, np.asarray(idx[: len(rows)], dtype=np.int64)], axis=1)
        check_closed(self.atoms, natoms, tuples)
        if tables is not None:
            A, B, types = (np.asarray(t) for t in tables)
            mask = np.zeros(natoms, dtype=bool)
            mask[self.atoms] = True
            cs, ce = np.unique(types[mask]), np.unique(types[~mask])
            if len(ce):
                a, b = A[np.ix_(cs, ce)], B[np.ix_(cs, ce)]
                if np.any((a > 0) & ~(b > 0)) or np.any(a < 0):
                    raise ValueError("Alchemical: a solute-environment pair has A > 0 >= B (or A < 0): sigma^6 = A / B does not exist")

    def solute_14(self, parameters, energies, dtype_np):
        """(pairs [M, 2], scee [M]) of the solute's 1-4 pairs whose charge part the context no longer sees."""
        if "1-4" not in energies or "electrostatics" not in energies:
            return np.zeros((0, 2), dtype=np.int32), np.zeros(0)
        p14 = getattr(parameters, "nonbonded_14_params", None)
        idx = _tuples(p14, 2)
        if len(idx) == 0:
            return np.zeros((0, 2), dtype=np.int32), np.zeros(0)
        mp = p14["map"].detach().cpu().numpy()
        prm = p14["params"].detach().cpu().numpy().astype(dtype_np)[mp[:, 1]]
        mask = np.isin(idx[:, 0], self.atoms)
        return np.ascontiguousarray(idx[mask]), np.ascontiguousarray(prm[mask, 3].astype(np.float64))

    def upload(self, lib, ctx, nreplicas, charges, classes, pair14, scee14, topology):
        """tmdhip_set_alchemical: `charges` / `classes` of the solute's atoms (ascending), rounded to the context's dtype."""
        lv, le = self.lambdas(nreplicas)
        d = L.AlchemicalDesc()
        d.struct_size = C.sizeof(L.AlchemicalDesc)
        d.enable = 1
        d.natoms, d.nreplicas = len(self.atoms), nreplicas
        tors = np.ascontiguousarray(np.concatenate([topology["torsion"], topology["improper"]], axis=0).astype(np.int32))
        keep = [np.array(self.atoms, dtype=np.int32, order="C"), np.array(charges, dtype=np.float64, order="C"),
                np.array(classes, dtype=np.int32, order="C"), lv, le, np.array(pair14, dtype=np.int32, order="C"),
                np.array(scee14, dtype=np.float64, order="C"), np.array(topology["bond"], dtype=np.int32, order="C"),
                np.array(topology["angle"], dtype=np.int32, order="C"), tors]
        ptrs = [a.ctypes.data_as(C.c_void_p) if a.size else C.c_void_p() for a in keep]
        (d.atoms_host, d.charges_host, d.classes_host, d.lambda_vdw_host, d.lambda_elec_host, d.pair14_host, d.scee14_host, d.bond_idx_host,
         d.angle_idx_host, d.torsion_idx_host) = ptrs
        d.alpha = self.alpha
        d.n14, d.nbonds, d.nangles, d.ntorsions = len(keep[5]), len(keep[7]), len(keep[8]), len(tors)
        L.check(lib.tmdhip_set_alchemical(ctx, C.byref(d)), "tmdhip_set_alchemical")
        del keep

    def sync(self, eng, owner):
        """Hand the solute to the context of `eng` when its copy is older (tmdhip_set_alchemical); `owner`: the `Forces`."""
        if eng.side_seen.get(self.side_name) == (id(self), self.version):
            return
        np_dtype = np.float32 if L.dtype_code(eng.dtype) == L.F32 else np.float64
        pair14, scee14 = self.solute_14(owner.par, owner.energies, np_dtype)
        self.upload(eng.lib, eng.ctx, eng.nreplicas, eng.alch_charges, eng.alch_classes, pair14, scee14,
                    self.topology(owner.par, owner.energies))
        eng.side_seen[self.side_name] = (id(self), self.version)

    def monitor_columns(self):
        return ("alchemical", "dudl_vdw", "dudl_elec")

    def monitor_row(self, k):
        return {"alchemical": float(self.energy[k, :3].sum()), "dudl_vdw": float(self.energy[k, 3]), "dudl_elec": float(self.energy[k, 4])}

    @classmethod
    def from_config(cls, cfg):
        """The `alchemical:` mapping of run.py: atoms, lambda_vdw, lambda_elec, alpha (and `states`, which run.py reads itself)."""
        unknown = set(cfg) - {"atoms", "lambda_vdw", "lambda_elec", "alpha", "states"}
        if unknown:
            raise ValueError(f"alchemical: unknown keys {sorted(unknown)}")
        if "atoms" not in cfg:
            raise ValueError("alchemical: `atoms` is required")
        return cls(np.asarray(cfg["atoms"], dtype=np.int64), cfg.get("lambda_vdw", 1.0), cfg.get("lambda_elec", 1.0), cfg.get("alpha", 0.5))
