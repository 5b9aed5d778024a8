"""Harmonic position and distance restraints with one target per replica.

    rs = Restraints(nreplicas)
    rs.add_position(atoms, reference, k)      # E = k |minimum image of (x - reference)|^2 / 2
    rs.add_distance(pairs, r0, k)             # E = k (r - r0)^2 / 2: the bond term with k0 = k / 2
    forces = Forces(..., restraints=rs)

`reference` is [M,3] or [R,M,3]; `k` and `r0` are a scalar, [M] or [R,M].  k = 0 switches an entry off for that replica.  The
tables live on the host in double; `set_distance_targets`, `set_position_reference` and `set_strengths` mark them dirty and
the next evaluation of a `Forces` that holds them uploads them (tmdhip_set_restraints), which is how an umbrella window's target
is moved between two `Integrator.step` calls.  `energy_forces` is the numpy model of the kernel (the tests' reference)."""

from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L


def min_image(d, box):
    """Minimum image of the difference vectors `d` [..., 3] in the orthorhombic box (edge lengths [3]); an edge of zero: no
    image along that axis.  The expression of restraint_math.h: d - box * rint(d / box)."""
    d = np.array(d, dtype=np.float64)
    box = np.asarray(box, dtype=np.float64).reshape(3)
    for c in range(3):
        if box[c] != 0.0:
            d[..., c] = d[..., c] - box[c] * np.rint(d[..., c] / box[c])
    return d


def build_rows(pos_atoms, pairs):
    """The per-atom rows the kernel walks, as tmdhip_set_restraints builds them: (atoms ascending, offsets, entries) with
    entries (kind, index, partner, sign): an atom's position entry (0, p, -1, 0) first, then its distance entries
    (1, d, partner, +1 for the first atom of pair d / -1 for the second) by restraint index."""
    pos_atoms = [int(a) for a in pos_atoms]
    pairs = [(int(i), int(j)) for i, j in pairs]
    atoms = sorted(set(pos_atoms) | {a for ij in pairs for a in ij})
    rows = {a: [] for a in atoms}
    for p, a in enumerate(pos_atoms):
        rows[a].append((0, p, -1, 0))
    for d, (i, j) in enumerate(pairs):
        rows[i].append((1, d, j, +1))
        rows[j].append((1, d, i, -1))
    off, ent = [0], []
    for a in atoms:
        ent.extend(rows[a])
        off.append(len(ent))
    return np.asarray(atoms, dtype=np.int32), np.asarray(off, dtype=np.int32), np.asarray(ent, dtype=np.int32).reshape(-1, 4)


class Restraints(L.SideTerm):
    side_name, side_width = "restraints", 2  # (position, distance)
    side_apply, side_energy = "tmdhip_restraint_apply", "tmdhip_restraint_energy"
    refusals = {
        "vmap": "compute() with restraints cannot run under torch.vmap (their targets are per replica of the context)",
        "batch": "restraints do not support atom groups (batch=): their targets are per replica",
        "barostat": "position restraints cannot run under barostat=: absolute references do not scale with the box "
                    "(distance restraints can)",
        "domain": "restraints cannot be domain-decomposed (a pair's atoms would straddle bricks, and atom indices change "
                  "at every migration)",
    }

    def __init__(self, nreplicas=1):
        if int(nreplicas) != nreplicas or nreplicas < 1:
            raise ValueError("Restraints: nreplicas must be a positive whole number")
        self.nreplicas = int(nreplicas)
        self.pos_atom = np.zeros(0, dtype=np.int32)
        self.pos_ref = np.zeros((self.nreplicas, 0, 3))
        self.pos_k = np.zeros((self.nreplicas, 0))
        self.dist_pair = np.zeros((0, 2), dtype=np.int32)
        self.dist_r0 = np.zeros((self.nreplicas, 0))
        self.dist_k = np.zeros((self.nreplicas, 0))
        self.version = 0  # bumped by whatever changes a table: an engine uploads when its copy is older

    # ------------------------------------------------------------------ the tables
    def _per_entry(self, v, m, what, nonneg=True):
        a = np.asarray(v, dtype=np.float64)
        if a.ndim == 0:
            a = np.full((self.nreplicas, m), float(a))
        elif a.shape == (m,):
            a = np.tile(a, (self.nreplicas, 1))
        elif a.shape != (self.nreplicas, m):
            raise ValueError(f"Restraints: {what} must be a scalar, [{m}] or [{self.nreplicas},{m}], got {a.shape}")
        if not np.all(np.isfinite(a)) or (nonneg and np.any(a < 0)):
            raise ValueError(f"Restraints: {what} must be finite" + (" and >= 0" if nonneg else ""))
        return np.ascontiguousarray(a)

    def _reference(self, ref, m):
        a = np.asarray(ref, dtype=np.float64)
        if a.shape == (m, 3):
            a = np.tile(a, (self.nreplicas, 1, 1))
        elif a.shape != (self.nreplicas, m, 3):
            raise ValueError(f"Restraints: reference must be [{m},3] or [{self.nreplicas},{m},3], got {a.shape}")
        if not np.all(np.isfinite(a)):
            raise ValueError("Restraints: reference must be finite")
        return np.ascontiguousarray(a)

    def add_position(self, atoms, reference, k):
        atoms = np.atleast_1d(np.asarray(atoms))
        if atoms.ndim != 1 or not np.issubdtype(atoms.dtype, np.integer) or np.any(atoms < 0):
            raise ValueError("Restraints.add_position: atoms must be non-negative whole numbers")
        both = np.concatenate([self.pos_atom, atoms.astype(np.int32)])
        if len(np.unique(both)) != len(both):
            raise ValueError("Restraints.add_position: an atom has one position restraint at most")
        m = len(atoms)
        ref, kk = self._reference(reference, m), self._per_entry(k, m, "k")
        self.pos_atom = both
        self.pos_ref = np.ascontiguousarray(np.concatenate([self.pos_ref, ref], axis=1))
        self.pos_k = np.ascontiguousarray(np.concatenate([self.pos_k, kk], axis=1))
        self.version += 1
        return self

    def add_distance(self, pairs, r0, k):
        pairs = np.asarray(pairs)
        if pairs.ndim == 1 and pairs.shape[0] == 2:
            pairs = pairs[None]
        if pairs.ndim != 2 or pairs.shape[1] != 2 or not np.issubdtype(pairs.dtype, np.integer) or np.any(pairs < 0):
            raise ValueError("Restraints.add_distance: pairs must be [M,2] non-negative whole numbers")
        if np.any(pairs[:, 0] == pairs[:, 1]):
            raise ValueError("Restraints.add_distance: the two atoms of a pair must differ")
        m = len(pairs)
        rr, kk = self._per_entry(r0, m, "r0"), self._per_entry(k, m, "k")
        self.dist_pair = np.ascontiguousarray(np.concatenate([self.dist_pair, pairs.astype(np.int32)], axis=0))
        self.dist_r0 = np.ascontiguousarray(np.concatenate([self.dist_r0, rr], axis=1))
        self.dist_k = np.ascontiguousarray(np.concatenate([self.dist_k, kk], axis=1))
        self.version += 1
        return self

    @property
    def npos(self):
        return len(self.pos_atom)

    @property
    def ndist(self):
        return len(self.dist_pair)

    def set_distance_targets(self, r0):
        self.dist_r0 = self._per_entry(r0, self.ndist, "r0")
        self.version += 1

    def set_position_reference(self, reference):
        self.pos_ref = self._reference(reference, self.npos)
        self.version += 1

    def set_strengths(self, position_k=None, distance_k=None):
        if position_k is not None:
            self.pos_k = self._per_entry(position_k, self.npos, "position_k")
        if distance_k is not None:
            self.dist_k = self._per_entry(distance_k, self.ndist, "distance_k")
        self.version += 1

    # ------------------------------------------------------------------ exchange of windows between replicas
    def exchange_parameters(self, nreplicas):
        """The four tables as they are, row a = state a, and `state_of_slot` (which `assign_states` keeps: the device tables
        are indexed by slot, `cross_energies` answers by state); None without entries."""
        if not (self.npos or self.ndist):
            return None
        if self.nreplicas != nreplicas:
            raise ValueError(f"restraints were made for {self.nreplicas} replicas, the exchange has {nreplicas}")
        return {"pos_ref": self.pos_ref.copy(), "pos_k": self.pos_k.copy(), "dist_r0": self.dist_r0.copy(),
                "dist_k": self.dist_k.copy(), "state_of_slot": np.arange(self.nreplicas, dtype=np.int64)}

    def cross_energies(self, owner, pos, box, snapshot):
        """Position plus distance energy of slot r's configuration under state a: tmdhip_restraint_states gives it under the
        row of every slot, and column a is the column of the slot that holds state a."""
        slot_of_state = np.argsort(snapshot["state_of_slot"])
        return owner.restraint_energies(pos, box).sum(axis=2)[:, slot_of_state]

    def assign_states(self, snapshot, state_of_slot):
        s = np.array(state_of_slot, dtype=np.int64)
        version = self.version
        if self.ndist:
            self.set_distance_targets(snapshot["dist_r0"][s])
        if self.npos:
            self.set_position_reference(snapshot["pos_ref"][s])
        self.set_strengths(snapshot["pos_k"][s] if self.npos else None, snapshot["dist_k"][s] if self.ndist else None)
        self.version = version + 1  # (one bump, one upload at the next evaluation)
        snapshot["state_of_slot"] = s

    def atoms(self):
        """Every restrained atom, ascending."""
        return np.unique(np.concatenate([self.pos_atom, self.dist_pair.reshape(-1)])).astype(np.int64)

    def check(self, natoms, masses=None, virtual_sites=None):
        """What a `Forces` refuses (ValueError): an index beyond the system, a restrained atom that is a virtual site or has
        no mass."""
        at = self.atoms()
        if len(at) and at[-1] >= natoms:
            raise ValueError(f"Restraints: atom {at[-1]} is beyond the system's {natoms} atoms")
        if masses is not None and len(at):
            m = np.asarray(masses, dtype=np.float64).reshape(-1)
            if np.any(~(m[at] > 0)):
                raise ValueError(f"Restraints: atom {at[~(m[at] > 0)][0]} is restrained and has no mass")
        if virtual_sites is not None and getattr(virtual_sites, "nsites", 0):
            hit = np.intersect1d(at, np.asarray(virtual_sites.sites))
            if len(hit):
                raise ValueError(f"Restraints: atom {hit[0]} is a virtual site (restrain its parents)")

    # ------------------------------------------------------------------ the model
    def energy_forces(self, pos, box):
        """The numpy model: `pos` [R,N,3] (or [N,3] with one replica), `box` edge lengths [3] or [R,3] (a [R,3,3] diagonal
        box is accepted).  Returns (energies [R,2] = (position, distance), forces [R,N,3]) in double."""
        pos = np.asarray(pos, dtype=np.float64)
        if pos.ndim == 2:
            pos = pos[None]
        R = pos.shape[0]
        if R != self.nreplicas:
            raise ValueError(f"Restraints.energy_forces: {R} replicas of positions for {self.nreplicas} replicas of tables")
        box = np.asarray(box, dtype=np.float64)
        if box.ndim == 3:
            box = np.stack([np.diag(b) for b in box])
        box = np.broadcast_to(box.reshape(-1, 3), (R, 3))
        E = np.zeros((R, 2))
        F = np.zeros_like(pos)
        for r in range(R):
            if self.npos:
                k = self.pos_k[r]
                d = min_image(pos[r, self.pos_atom] - self.pos_ref[r], box[r])
                d[k == 0] = 0.0
                E[r, 0] = np.sum(0.5 * k * np.sum(d * d, axis=1))
                np.add.at(F[r], self.pos_atom, -k[:, None] * d)
            if self.ndist:
                k, r0 = self.dist_k[r], self.dist_r0[r]
                i, j = self.dist_pair[:, 0], self.dist_pair[:, 1]
                d = min_image(pos[r, i] - pos[r, j], box[r])
                d[k == 0] = 0.0
                rr = np.sqrt(np.sum(d * d, axis=1))
                x = rr - r0
                E[r, 1] = np.sum(0.5 * k * (x * x))
                with np.errstate(invalid="ignore", divide="ignore"):
                    s = np.where(rr > 0, (-k * x) / rr, 0.0)
                fi = s[:, None] * d
                # (one pass in restraint order, both ends of a restraint together: the order in which the kernel's thread adds)
                np.add.at(F[r], self.dist_pair.reshape(-1), np.stack([fi, -fi], axis=1).reshape(-1, 3))
        return E, F

    # ------------------------------------------------------------------ the device tables
    def descriptor(self):
        """(tmdhip_restraint_desc, the arrays it points at)."""
        d = L.RestraintDesc()
        d.struct_size = C.sizeof(L.RestraintDesc)
        d.enable = 1 if (self.npos or self.ndist) else 0
        d.nreplicas, d.npos, d.ndist = self.nreplicas, self.npos, self.ndist
        # (copies: what the library reads is never the object's own state)
        keep = [np.array(self.pos_atom, dtype=np.int32, order="C"), np.array(self.pos_ref, dtype=np.float64, order="C"),
                np.array(self.pos_k, dtype=np.float64, order="C"), np.array(self.dist_pair, dtype=np.int32, order="C"),
                np.array(self.dist_r0, dtype=np.float64, order="C"), np.array(self.dist_k, dtype=np.float64, order="C")]
        ptrs = [a.ctypes.data_as(C.c_void_p) if a.size else C.c_void_p() for a in keep]
        d.pos_atom_host, d.pos_ref_host, d.pos_k_host, d.dist_pair_host, d.dist_r0_host, d.dist_k_host = ptrs
        return d, keep

    def upload(self, lib, ctx):
        d, keep = self.descriptor()
        L.check(lib.tmdhip_set_restraints(ctx, C.byref(d)), "tmdhip_set_restraints")
        del keep

    def refusal(self, what):
        """(Distance restraints scale with the box: only absolute references are refused under a barostat.)"""
        return None if (what == "barostat" and not self.npos) else self.refusals.get(what)

    def sync(self, eng, owner=None):
        """Upload the tables when the copy of `eng`'s context is older (tmdhip_set_restraints)."""
        if eng.side_seen.get(self.side_name) == (id(self), self.version):
            return
        if self.nreplicas != eng.nreplicas:
            raise ValueError(f"restraints were made for {self.nreplicas} replicas, the positions have {eng.nreplicas}")
        self.upload(eng.lib, eng.ctx)
        eng.side_seen[self.side_name] = (id(self), self.version)

    @classmethod
    def from_npz(cls, path, nreplicas):
        """The `restraints:` file of run.py: arrays named as the fields of tmdhip_restraint_desc without `_host`
        (pos_atom, pos_ref, pos_k, dist_pair, dist_r0, dist_k); per-replica leading axes are optional."""
        z = np.load(path)
        rs = cls(nreplicas)
        if "pos_atom" in z.files and len(z["pos_atom"]):
            rs.add_position(z["pos_atom"], z["pos_ref"], z["pos_k"])
        if "dist_pair" in z.files and len(z["dist_pair"]):
            rs.add_distance(z["dist_pair"], z["dist_r0"], z["dist_k"])
        return rs
