"""Harmonic, optionally flat-bottomed restraints on the distance, angle and dihedral between centres of groups of atoms, with
targets, strengths and widths per replica.

    gr = GroupRestraints(nreplicas)
    p = gr.add_group(pocket_atoms)                 # weights=None: the masses of the Forces' parameters; or an explicit [n] > 0
    l = gr.add_group(ligand_atoms)
    gr.add_distance((p, l), r0, k, flat=0.0)       # r0, k, flat: scalar or [R]; returns the restraint's index
    gr.add_angle((g1, g2, g3), theta0, k, flat=0.0)
    gr.add_dihedral((g1, g2, g3, g4), phi0, k, flat=0.0)
    forces = Forces(..., group_restraints=gr)

The centre of a group with atoms a0, a1, ... in the order given is X = x_a0 + sum_a w_a mi(x_a - x_a0), w_a = W_a / sum W, `mi`
the minimum image.  PRECONDITION: every atom of a group lies within half a box edge of the group's first atom along every
periodic axis (`check_extent` says whether it holds; run.py calls it on the start configuration).  A group of one atom is that
atom.  With delta = s - s0 (wrapped into [-pi, pi] for a dihedral) and u = sign(delta) max(|delta| - flat, 0): E = k u^2 / 2.
k = 0 switches an entry off for that replica.  `energy_forces` is the numpy model of the kernels (the tests' reference)."""

from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _lib as L
from .metadynamics import _dot, cv_dihedral
from .restraints import min_image

DISTANCE, ANGLE, DIHEDRAL = 0, 1, 2
KIND_NAMES = ("distance", "angle", "dihedral")
STANDARD_VOLUME = 1660.5392  # A^3: one molecule at 1 mol / l


def flat_well(delta, flat):
    """u = sign(delta) max(|delta| - flat, 0)."""
    m = abs(delta) - flat
    um = m if m > 0.0 else 0.0
    return -um if delta < 0.0 else um


def restraint_terms(kind, X, box, s0, k, flat):
    """One restraint on its centres X [arity, 3] in double, the operations of group_math.h in their order: (E, F [4, 3] with
    F[a] = -dE/dX_a, s)."""
    F = np.zeros((4, 3))
    if kind == DISTANCE:
        d = min_image(X[0] - X[1], box)
        r = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
        u = flat_well(r - s0, flat)
        if r > 0.0:
            s = (-k * u) / r
            F[0] = s * d
            F[1] = -F[0]
        return 0.5 * k * (u * u), F, r
    if kind == ANGLE:
        u, v = min_image(X[0] - X[1], box), min_image(X[2] - X[1], box)
        nu, nv = np.sqrt(_dot(u, u)), np.sqrt(_dot(v, v))
        co = 1.0
        if nu > 0.0 and nv > 0.0:
            co = _dot(u, v) / (nu * nv)
        co = 1.0 if co > 1.0 else (-1.0 if co < -1.0 else co)
        theta = math.acos(co)
        w = flat_well(theta - s0, flat)
        si = np.sqrt(1.0 - co * co)
        if nu > 0.0 and nv > 0.0 and si > 0.0:
            fa, fc = (k * w) / (nu * si), (k * w) / (nv * si)
            uh, vh = u / nu, v / nv
            F[0] = fa * (vh - co * uh)
            F[2] = fc * (uh - co * vh)
            F[1] = -F[0] - F[2]
        return 0.5 * k * (w * w), F, theta
    phi, g = cv_dihedral(X, box)
    delta = phi - s0
    delta = delta - (2.0 * np.pi) * np.rint(delta / (2.0 * np.pi))
    u = flat_well(delta, flat)
    F[:] = (-k * u) * g
    return 0.5 * k * (u * u), F, phi


def fixed_order_sum(terms):
    """The sum of `terms` [n, 3] in the order of the centre kernel (group_restraint.hip, the fixed-order sum of reduce.h): lane
    t of a block of 256 adds terms t, t + 256, ... from 0.0; the xor butterfly of each wave of 64 lanes; the four wave results
    meet pairwise, (p0 + p1) + (p2 + p3)."""
    terms = np.asarray(terms, dtype=np.float64)
    acc = np.zeros((256, 3))
    for lo in range(0, len(terms), 256):
        part = terms[lo : lo + 256]
        acc[: len(part)] = acc[: len(part)] + part
    lane = np.arange(64)
    wave = []
    for w in range(4):
        v = acc[64 * w : 64 * w + 64]
        for o in (32, 16, 8, 4, 2, 1):
            v = v + v[lane ^ o]
        wave.append(v[0])
    return (wave[0] + wave[1]) + (wave[2] + wave[3])


class GroupRestraints(L.SideTerm):
    side_name, side_width = "group_restraints", 3  # (distance, angle, dihedral)
    side_apply, side_energy = "tmdhip_group_restraint_apply", "tmdhip_group_restraint_energy"
    refusals = {
        "vmap": "compute() with group restraints cannot run under torch.vmap (their targets are per replica of the context)",
        "batch": "group restraints do not support atom groups (batch=): their targets are per replica",
        "barostat": "group restraints cannot run under barostat=: the virial of the centres is not computed",
        "pressure": "the pressure is not available with group restraints: the virial of the centres is not computed",
        "update_atoms": "update_atoms() is not available with group restraints: the groups name atoms by index",
        "domain": "group restraints cannot be domain-decomposed (a group's atoms would straddle bricks, and atom indices "
                  "change at every migration)",
    }

    def __init__(self, nreplicas=1):
        if int(nreplicas) != nreplicas or nreplicas < 1:
            raise ValueError("GroupRestraints: nreplicas must be a positive whole number")
        self.nreplicas = int(nreplicas)
        self.group_atoms = []  # per group: int32 [n] in the order given
        self.group_weights = []  # per group: float64 [n] > 0, or None = the masses
        self.kind = np.zeros(0, dtype=np.int32)
        self.groups = np.zeros((0, 4), dtype=np.int32)  # -1 padded
        self.target = np.zeros((self.nreplicas, 0))
        self.k = np.zeros((self.nreplicas, 0))
        self.flat = np.zeros((self.nreplicas, 0))
        self.masses = None  # what a Forces hands over (check): the default weights
        self.version = 0
        self._boresch = None  # the indices of the six restraints `boresch` built (r, thetaA, thetaB, phiA, phiB, phiC)

    # ------------------------------------------------------------------ the tables
    @property
    def ngroups(self):
        return len(self.group_atoms)

    @property
    def nrestraints(self):
        return len(self.kind)

    def add_group(self, atoms, weights=None):
        atoms = np.atleast_1d(np.asarray(atoms))
        if atoms.ndim != 1 or len(atoms) == 0 or not np.issubdtype(atoms.dtype, np.integer) or np.any(atoms < 0):
            raise ValueError("GroupRestraints.add_group: atoms must be a non-empty list of non-negative whole numbers")
        if len(np.unique(atoms)) != len(atoms):
            raise ValueError("GroupRestraints.add_group: an atom is named twice")
        if weights is not None:
            weights = np.array(weights, dtype=np.float64)
            if weights.shape != atoms.shape or not np.all(np.isfinite(weights)) or np.any(~(weights > 0)):
                raise ValueError(f"GroupRestraints.add_group: weights must be [{len(atoms)}], finite and > 0")
        self.group_atoms.append(atoms.astype(np.int32))
        self.group_weights.append(weights)
        self.version += 1
        return self.ngroups - 1

    def _per_replica(self, v, what, nonneg):
        a = np.asarray(v, dtype=np.float64)
        if a.ndim == 0:
            a = np.full(self.nreplicas, float(a))
        elif a.shape != (self.nreplicas,):
            raise ValueError(f"GroupRestraints: {what} must be a scalar or [{self.nreplicas}], got {a.shape}")
        if not np.all(np.isfinite(a)) or (nonneg and np.any(a < 0)):
            raise ValueError(f"GroupRestraints: {what} must be finite" + (" and >= 0" if nonneg else ""))
        return a

    def _add(self, kind, groups, target, k, flat):
        name = KIND_NAMES[kind]
        g = np.asarray(groups)
        if g.shape != (kind + 2,) or not np.issubdtype(g.dtype, np.integer):
            raise ValueError(f"GroupRestraints.add_{name}: wrong number of groups: {kind + 2} group indices are needed")
        if np.any(g < 0) or np.any(g >= self.ngroups):
            raise ValueError(f"GroupRestraints.add_{name}: a group index is out of range")
        if len(np.unique(g)) != len(g):
            raise ValueError(f"GroupRestraints.add_{name}: a group is named twice")
        t, kk, fl = self._per_replica(target, "the target", False), self._per_replica(k, "k", True), self._per_replica(flat, "flat", True)
        if kind == ANGLE and (np.any(t < 0) or np.any(t > np.pi)):
            raise ValueError("GroupRestraints.add_angle: the target must lie in [0, pi]")
        row = np.full(4, -1, dtype=np.int32)
        row[: kind + 2] = g
        self.kind = np.append(self.kind, np.int32(kind)).astype(np.int32)
        self.groups = np.ascontiguousarray(np.concatenate([self.groups, row[None]], axis=0))
        self.target = np.ascontiguousarray(np.concatenate([self.target, t[:, None]], axis=1))
        self.k = np.ascontiguousarray(np.concatenate([self.k, kk[:, None]], axis=1))
        self.flat = np.ascontiguousarray(np.concatenate([self.flat, fl[:, None]], axis=1))
        self.version += 1
        return self.nrestraints - 1

    def add_distance(self, groups, r0, k, flat=0.0):
        return self._add(DISTANCE, groups, r0, k, flat)

    def add_angle(self, groups, theta0, k, flat=0.0):
        return self._add(ANGLE, groups, theta0, k, flat)

    def add_dihedral(self, groups, phi0, k, flat=0.0):
        return self._add(DIHEDRAL, groups, phi0, k, flat)

    def _table(self, v, what, nonneg):
        a = np.asarray(v, dtype=np.float64)
        m = self.nrestraints
        if a.ndim == 0:
            a = np.full((self.nreplicas, m), float(a))
        elif a.shape == (m,):
            a = np.tile(a, (self.nreplicas, 1))
        elif a.shape != (self.nreplicas, m):
            raise ValueError(f"GroupRestraints: {what} must be a scalar, [{m}] or [{self.nreplicas},{m}], got {a.shape}")
        if not np.all(np.isfinite(a)) or (nonneg and np.any(a < 0)):
            raise ValueError(f"GroupRestraints: {what} must be finite" + (" and >= 0" if nonneg else ""))
        return np.ascontiguousarray(a)

    def set_targets(self, target):
        t = self._table(target, "the targets", False)
        ang = self.kind == ANGLE
        if np.any(t[:, ang] < 0) or np.any(t[:, ang] > np.pi):
            raise ValueError("GroupRestraints: an angle target must lie in [0, pi]")
        self.target = t
        self.version += 1

    def set_strengths(self, k):
        self.k = self._table(k, "k", True)
        self.version += 1

    def set_flat(self, flat):
        self.flat = self._table(flat, "flat", True)
        self.version += 1

    # ------------------------------------------------------------------ exchange of windows between replicas
    def exchange_parameters(self, nreplicas):
        if not self.nrestraints:
            return None
        if self.nreplicas != nreplicas:
            raise ValueError(f"group restraints were made for {self.nreplicas} replicas, the exchange has {nreplicas}")
        return {"target": self.target.copy(), "k": self.k.copy(), "flat": self.flat.copy(),
                "state_of_slot": np.arange(self.nreplicas, dtype=np.int64)}

    def cross_energies(self, owner, pos, box, snapshot):
        """The term's energy of slot r's configuration under state a: tmdhip_group_restraint_states gives it under the row of
        every slot, and column a is the column of the slot that holds state a."""
        slot_of_state = np.argsort(snapshot["state_of_slot"])
        return owner.group_restraint_energies(pos, box).sum(axis=2)[:, slot_of_state]

    def assign_states(self, snapshot, state_of_slot):
        s = np.array(state_of_slot, dtype=np.int64)
        self.target = np.ascontiguousarray(snapshot["target"][s])
        self.k = np.ascontiguousarray(snapshot["k"][s])
        self.flat = np.ascontiguousarray(snapshot["flat"][s])
        self.version += 1  # (one bump, one upload at the next evaluation)
        snapshot["state_of_slot"] = s

    # ------------------------------------------------------------------ what a Forces checks and hands over
    def atoms(self):
        """Every atom of a group, ascending."""
        if not self.ngroups:
            return np.zeros(0, dtype=np.int64)
        return np.unique(np.concatenate(self.group_atoms)).astype(np.int64)

    def check(self, natoms, masses=None, virtual_sites=None):
        """What a `Forces` refuses (ValueError): an index beyond the system, a group atom that is a virtual site or has no
        mass.  The masses become the default weights."""
        at = self.atoms()
        if len(at) and at[-1] >= natoms:
            raise ValueError(f"GroupRestraints: atom {at[-1]} is beyond the system's {natoms} atoms")
        if virtual_sites is not None and getattr(virtual_sites, "nsites", 0):
            hit = np.intersect1d(at, np.asarray(virtual_sites.sites))
            if len(hit):
                raise ValueError(f"GroupRestraints: atom {hit[0]} is a virtual site (name its parents)")
        if masses is not None:
            m = np.array(masses, dtype=np.float64).reshape(-1)
            if len(at) and np.any(~(m[at] > 0)):
                raise ValueError(f"GroupRestraints: atom {at[~(m[at] > 0)][0]} belongs to a group and has no mass")
            if self.masses is None or not np.array_equal(self.masses, m):
                self.masses = m
                self.version += 1

    def raw_weights(self, g):
        """The raw weights W of group g: the explicit ones, or the masses a `Forces` handed over (`masses` may be set by hand)."""
        if self.group_weights[g] is not None:
            return self.group_weights[g]
        if self.masses is None:
            raise ValueError("GroupRestraints: a group without explicit weights needs masses (pass the object to Forces, or set .masses)")
        return np.asarray(self.masses, dtype=np.float64)[self.group_atoms[g]]

    def weights(self, g):
        """The normalised weights of group g, the sum taken in member order (as the library normalises)."""
        W = self.raw_weights(g)
        total = 0.0
        for x in W:
            total += float(x)
        return W / total

    # ------------------------------------------------------------------ the model
    def _boxes(self, box, R):
        box = np.asarray(box, dtype=np.float64)
        if box.ndim == 3:
            box = np.stack([np.diag(b) for b in box])
        return np.broadcast_to(box.reshape(-1, 3), (R, 3))

    def _positions(self, pos):
        pos = np.asarray(pos, dtype=np.float64)
        if pos.ndim == 2:
            pos = pos[None]
        if pos.shape[0] != self.nreplicas:
            raise ValueError(f"GroupRestraints: {pos.shape[0]} replicas of positions for {self.nreplicas} replicas of tables")
        return pos

    def centres(self, pos, box):
        """[R, G, 3] in double: X_g = x_a0 + sum_a w_a mi(x_a - x_a0), the sum taken in the centre kernel's order
        (`fixed_order_sum`), so that the model's centres are the kernel's."""
        pos = self._positions(pos)
        R = pos.shape[0]
        box = self._boxes(box, R)
        X = np.zeros((R, self.ngroups, 3))
        for g, at in enumerate(self.group_atoms):
            w = self.weights(g)
            for r in range(R):
                x0 = pos[r, at[0]]
                X[r, g] = x0 + fixed_order_sum(w[:, None] * min_image(pos[r, at] - x0, box[r]))
        return X

    def check_extent(self, pos, box):
        """Whether the precondition holds for `pos` [R,N,3] or [N,3] in `box`: every atom of a group within half a box edge
        of the group's first atom along every periodic axis (judged on the raw difference, without an image)."""
        pos = np.asarray(pos, dtype=np.float64)
        if pos.ndim == 2:
            pos = pos[None]
        box = self._boxes(box, pos.shape[0])
        for at in self.group_atoms:
            for r in range(pos.shape[0]):
                d = np.abs(min_image(pos[r, at] - pos[r, at[0]], box[r]))
                per = box[r] != 0
                if np.any(d[:, per] >= 0.5 * box[r][per] * (1.0 - 1e-12)):
                    return False
        return True

    def uses(self):
        """Per group: [(restraint, role)] by ascending restraint index."""
        per = [[] for _ in range(self.ngroups)]
        for m in range(self.nrestraints):
            for a in range(self.kind[m] + 2):
                per[self.groups[m, a]].append((m, a))
        return per

    def build_rows(self):
        """The rows the force kernel walks, as tmdhip_set_group_restraints builds them: (use_off [G+1], use [.,2] = (restraint,
        role), atoms ascending, mem_off, mem [.,2] = (group, place in the concatenated member list))."""
        per = self.uses()
        use_off, use = [0], []
        for g in range(self.ngroups):
            use.extend(per[g])
            use_off.append(len(use))
        off = np.concatenate([[0], np.cumsum([len(a) for a in self.group_atoms])]).astype(np.int64)
        rows = {}
        for g, at in enumerate(self.group_atoms):
            if per[g]:
                for j, a in enumerate(at):
                    rows.setdefault(int(a), []).append((g, int(off[g] + j)))
        atoms = sorted(rows)
        mem_off, mem = [0], []
        for a in atoms:
            mem.extend(rows[a])
            mem_off.append(len(mem))
        i32 = lambda v, w: np.asarray(v, dtype=np.int32).reshape(-1, w) if w else np.asarray(v, dtype=np.int32)
        return i32(use_off, 0), i32(use, 2), i32(atoms, 0), i32(mem_off, 0), i32(mem, 2)

    def energy_forces(self, pos, box, k_scale=1.0):
        """The numpy model: `pos` [R,N,3] (or [N,3] with one replica), `box` edge lengths [3] or [R,3] (a [R,3,3] diagonal box
        is accepted).  Returns (energies [R,3] = (distance, angle, dihedral), forces [R,N,3]) in double.  Per atom the sum runs
        over its memberships by ascending group and, within a group, over the restraints by ascending index.  `k_scale`
        multiplies every k (the tests' control)."""
        pos = self._positions(pos)
        R = pos.shape[0]
        box = self._boxes(box, R)
        X = self.centres(pos, box)
        E = np.zeros((R, 3))
        F = np.zeros_like(pos)
        per = self.uses()
        w = [self.weights(g) for g in range(self.ngroups)]
        for r in range(R):
            fc = {}
            for m in range(self.nrestraints):
                k = self.k[r, m] * k_scale
                if not k > 0.0:
                    continue
                kind = int(self.kind[m])
                e, f, _ = restraint_terms(kind, X[r, self.groups[m, : kind + 2]], box[r], self.target[r, m], k, self.flat[r, m])
                E[r, kind] += e
                fc[m] = f
            G = np.zeros((self.ngroups, 3))
            for g in range(self.ngroups):
                for m, a in per[g]:
                    if m in fc:
                        G[g] += fc[m][a]
            for g, at in enumerate(self.group_atoms):  # (ascending group: the order in which an atom's thread adds)
                if per[g]:
                    F[r, at] += w[g][:, None] * G[g]
        return E, F

    def values(self, pos, box):
        """The collective variables [R, M]."""
        pos = self._positions(pos)
        box = self._boxes(box, pos.shape[0])
        X = self.centres(pos, box)
        out = np.zeros((pos.shape[0], self.nrestraints))
        for r in range(pos.shape[0]):
            for m in range(self.nrestraints):
                kind = int(self.kind[m])
                out[r, m] = restraint_terms(kind, X[r, self.groups[m, : kind + 2]], box[r], 0.0, 0.0, 0.0)[2]
        return out

    # ------------------------------------------------------------------ the device tables
    def descriptor(self):
        """(tmdhip_group_restraint_desc, the arrays it points at)."""
        d = L.GroupRestraintDesc()
        d.struct_size = C.sizeof(L.GroupRestraintDesc)
        d.enable = 1 if self.nrestraints else 0
        d.nreplicas, d.ngroups, d.nrestraints = self.nreplicas, self.ngroups, self.nrestraints
        off = np.concatenate([[0], np.cumsum([len(a) for a in self.group_atoms])]).astype(np.int32)
        atoms = np.concatenate(self.group_atoms).astype(np.int32) if self.ngroups else np.zeros(0, dtype=np.int32)
        W = (np.concatenate([self.raw_weights(g) for g in range(self.ngroups)]).astype(np.float64) if (self.ngroups and d.enable)
             else np.zeros(0))
        # (copies: what the library reads is never the object's own state)
        keep = [np.ascontiguousarray(off), np.ascontiguousarray(atoms), np.ascontiguousarray(W), np.array(self.kind, dtype=np.int32, order="C"),
                np.array(self.groups, dtype=np.int32, order="C"), np.array(self.target, dtype=np.float64, order="C"),
                np.array(self.k, dtype=np.float64, order="C"), np.array(self.flat, dtype=np.float64, order="C")]
        ptrs = [a.ctypes.data_as(C.c_void_p) if a.size else C.c_void_p() for a in keep]
        (d.group_off_host, d.member_atom_host, d.member_weight_host, d.kind_host, d.groups_host, d.target_host, d.k_host,
         d.flat_host) = ptrs
        return d, keep

    def upload(self, lib, ctx):
        d, keep = self.descriptor()
        L.check(lib.tmdhip_set_group_restraints(ctx, C.byref(d)), "tmdhip_set_group_restraints")
        del keep

    def sync(self, eng, owner=None):
        """Upload the tables when the copy of `eng`'s context is older (tmdhip_set_group_restraints)."""
        if eng.side_seen.get(self.side_name) == (id(self), self.version):
            return
        if self.nreplicas != eng.nreplicas:
            raise ValueError(f"group restraints were made for {self.nreplicas} replicas, the positions have {eng.nreplicas}")
        self.upload(eng.lib, eng.ctx)
        eng.side_seen[self.side_name] = (id(self), self.version)

    def monitor_columns(self):
        return (self.side_name,)

    @classmethod
    def from_npz(cls, path, nreplicas):
        """The `group_restraints:` file of run.py: group_off [G+1], member_atom, optionally member_weight (absent: the
        masses), kind [M], groups [M,4] (-1 padded), target, k and optionally flat, each a scalar, [M] or [R,M]."""
        z = np.load(path)
        gr = cls(nreplicas)
        off, atoms = z["group_off"], z["member_atom"]
        W = z["member_weight"] if "member_weight" in z.files else None
        for g in range(len(off) - 1):
            gr.add_group(atoms[off[g] : off[g + 1]], None if W is None else W[off[g] : off[g + 1]])
        kind, groups = np.atleast_1d(z["kind"]), np.atleast_2d(z["groups"])
        M = len(kind)

        def table(name, default=None):
            if name not in z.files:
                return np.full((nreplicas, M), default)
            a = np.asarray(z[name], dtype=np.float64)
            return np.broadcast_to(a, (nreplicas, M)) if a.ndim < 2 else a

        t, k, fl = table("target"), table("k"), table("flat", 0.0)
        for m in range(M):
            gr._add(int(kind[m]), groups[m, : int(kind[m]) + 2], t[:, m], k[:, m], fl[:, m])
        return gr

    # ------------------------------------------------------------------ the Boresch set
    @classmethod
    def boresch(cls, nreplicas, receptor, ligand, r0, theta_a0, theta_b0, phi_a0, phi_b0, phi_c0, k_r, k_theta, k_phi):
        """Six single-atom groups (P1, P2, P3, L1, L2, L3) and the six restraints of Boresch et al. (2003): r = P1-L1,
        thetaA = P2-P1-L1, thetaB = P1-L1-L2, phiA = P3-P2-P1-L1, phiB = P2-P1-L1-L2, phiC = P1-L1-L2-L3."""
        if len(receptor) != 3 or len(ligand) != 3:
            raise ValueError("GroupRestraints.boresch: three receptor and three ligand atoms are needed")
        gr = cls(nreplicas)
        P1, P2, P3 = (gr.add_group([int(a)], weights=[1.0]) for a in receptor)  # (a group of one atom is that atom)
        L1, L2, L3 = (gr.add_group([int(a)], weights=[1.0]) for a in ligand)
        gr._boresch = (gr.add_distance((P1, L1), r0, k_r), gr.add_angle((P2, P1, L1), theta_a0, k_theta),
                       gr.add_angle((P1, L1, L2), theta_b0, k_theta), gr.add_dihedral((P3, P2, P1, L1), phi_a0, k_phi),
                       gr.add_dihedral((P2, P1, L1, L2), phi_b0, k_phi), gr.add_dihedral((P1, L1, L2, L3), phi_c0, k_phi))
        return gr

    def boresch_standard_state(self, temperature):
        """The analytic correction per replica [R] in kcal/mol for releasing the Boresch set into the standard volume:
        -kT ln[8 pi^2 V0 sqrt(K_r K_thA K_thB K_phA K_phB K_phC) / (r0^2 sin thA0 sin thB0 (2 pi kT)^3)], V0 = 1660.5392 A^3."""
        from .integrator import BOLTZMAN

        if self._boresch is None or self.nrestraints != 6 or self.ngroups != 6:
            raise ValueError("boresch_standard_state(): the set was not built by GroupRestraints.boresch")
        idx = list(self._boresch)
        if np.any(self.flat[:, idx] > 0):
            raise ValueError("boresch_standard_state(): the analytic correction is for flat = 0")
        K, t = self.k[:, idx], self.target[:, idx]
        if np.any(~(K > 0)):
            raise ValueError("boresch_standard_state(): every k must be > 0")
        kT = BOLTZMAN * float(temperature)
        num = 8.0 * np.pi**2 * STANDARD_VOLUME * np.sqrt(np.prod(K, axis=1))
        den = t[:, 0] ** 2 * np.sin(t[:, 1]) * np.sin(t[:, 2]) * (2.0 * np.pi * kT) ** 3
        return -kT * np.log(num / den)
