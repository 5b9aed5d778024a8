"""Seeded systems for the Verlet-list build's tests (test_list_systems_host.py, test_gpu_list_build.py): what the cubic,
molecule-ordered lattices of the rest of the suite cannot show — per-axis cell counts, empty cells and a density step, atom
numbers that alias in the build's exclusion bitmap (key = original index mod 2048), and an open box a thousand cells long.

Every builder returns a `ListSystem`.  Nothing here needs a GPU."""

from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from torchmd_amd.builders import _random_rotations, argon_forcefield, water_forcefield
from torchmd_amd.io import Topology

CUTOFF = 9.0
SKIN = 1.2  # the library's default (asserted against stats()["skin"] by the GPU tests)
RLIST = CUTOFF + SKIN  # the largest pair radius when some weight is 1 and TMDHIP_VSKIN=0 (context.hip: tmdhip_set_skin_weights)
# per-axis stretch of the lattice constant: the edges of a box are no multiples of one another, nor of one spacing
STRETCH = np.array([1.0, 1.01, 0.99])
WATER_A = (1.0 / 0.0334) ** (1.0 / 3.0)  # builders.tip3p_box: 3.105 A

# molecule counts per axis and the cells they plan (asserted on the GPU; cell edge >= RLIST / m):
BOX_M2 = (9, 12, 20)   # m = 2: (5, 7, 12) — and (7, 12, 5), (12, 5, 7) for the two other placements of the short axis
BOX_M3 = (8, 11, 15)   # m = 3: (7, 10, 13)
BOX_ALL = (10, 12, 15)  # m = 1: (3, 3, 4) at 150 atoms per cell, m = 2: (6, 7, 9), m = 3: (9, 11, 13)
# Seeds (the slab and the permuted box are the m = 2 box).  The electrostatic energy of randomly oriented waters is what is left
# of +-35 kcal/mol pair terms, some hundred kcal/mol at these sizes, and the GPU tests hold it to the parity bar ERTOL x EFAC x |E|
# against the oracle in the context's precision.  That comparison means something only where the oracle resolves the bar: its own
# fp32 error (fp32 against fp64 on the same values, ~4e-3 kcal/mol here) may use at most half of it, which
# test_list_systems_host.py asserts for every system.  Seed 12 on the m = 3 box fails that (E = -5.93: bar 3.6e-4, the oracle's
# fp32 error 3.7e-3); 13 is the next seed.
SEEDS = {"m2": 11, "slab": 11, "permuted": 11, "m3": 13, "all": 13}


@dataclass
class ListSystem:
    name: str
    mol: Topology
    pos: np.ndarray  # [N, 3] float64
    box: np.ndarray  # [3]; all zero: open
    kind: str  # "water" | "argon"
    meta: dict = field(default_factory=dict)

    @property
    def natoms(self):
        return len(self.pos)

    def par(self, dtype):
        from torchmd_amd.parameters import Parameters

        ff = water_forcefield(self.mol) if self.kind == "water" else argon_forcefield(self.mol)
        terms = ["lj", "electrostatics"] + (["bonds", "angles"] if self.kind == "water" else [])
        return Parameters(ff, self.mol, terms, precision=dtype)

    def exclusions(self):
        """[E, 2] excluded pairs, from the topology alone (bonds and angle ends: what Parameters.get_exclusions returns)"""
        ex = [np.asarray(self.mol.bonds).reshape(-1, 2)]
        if len(self.mol.angles):
            ex.append(np.asarray(self.mol.angles)[:, [0, 2]])
        return np.concatenate(ex).astype(np.int64)


def expected_cells(box, m, rlist=RLIST):
    """Cells per axis of stencil half-width m (grid_plan.h; for the host tests — the GPU tests assert stats()["ncell"])"""
    return tuple(int(v) for v in np.minimum(np.floor(np.asarray(box) / (rlist / m)), 1024))


def _water(nx, ny, nz, seed, jitter=0.2):
    rng = np.random.default_rng(seed)
    a = WATER_A * STRETCH
    gx, gy, gz = np.arange(nx), np.arange(ny), np.arange(nz)
    sites = np.stack(np.meshgrid(gx, gy, gz, indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float64)
    nmol = len(sites)
    oxy = sites * a + a / 2 + rng.uniform(-jitter, jitter, size=(nmol, 3))
    r, th = 0.9572, np.deg2rad(104.52)
    h1 = np.array([r * np.sin(th / 2), 0.0, r * np.cos(th / 2)])
    h2 = np.array([-r * np.sin(th / 2), 0.0, r * np.cos(th / 2)])
    rot = _random_rotations(rng, nmol)
    pos = np.empty((nmol, 3, 3))
    pos[:, 0] = oxy
    pos[:, 1] = oxy + rot @ h1
    pos[:, 2] = oxy + rot @ h2
    return pos, a * np.array([nx, ny, nz]), rng


def _water_system(name, molpos, box, perm=None):
    """molpos [nmol, 3, 3] (O, H1, H2).  perm: new index of old atom i, or None for molecule order."""
    nmol = len(molpos)
    n = 3 * nmol
    base = 3 * np.arange(nmol)
    bonds = np.stack([np.stack([base, base + 1], 1), np.stack([base, base + 2], 1), np.stack([base + 1, base + 2], 1)], 1).reshape(-1, 2)
    angles = np.stack([base + 1, base, base + 2], axis=1)
    atomtype = np.tile(np.array(["OT", "HT", "HT"], dtype=object), nmol)
    charge = np.tile(np.array([-0.834, 0.417, 0.417], dtype=np.float32), nmol)
    masses = np.tile(np.array([15.9994, 1.008, 1.008], dtype=np.float32), nmol)
    pos = molpos.reshape(-1, 3)
    meta = {}
    if perm is not None:
        inv = np.argsort(perm)  # old index of new atom k
        atomtype, charge, masses, pos = atomtype[inv], charge[inv], masses[inv], pos[inv]
        bonds, angles = perm[bonds], perm[angles]
        meta["perm"] = perm
    mol = Topology(atomtype=atomtype, charge=charge, masses=masses, bonds=bonds.astype(np.int64), angles=angles.astype(np.int64))
    assert len(pos) == n
    return ListSystem(name, mol, np.ascontiguousarray(pos), np.asarray(box, dtype=np.float64), "water", meta)


def water_box(nx, ny, nz, seed, permute=False):
    """nx x ny x nz TIP3P molecules at the density, jitter and orientations of builders.tip3p_box, the lattice constant
    stretched per axis by STRETCH.  permute: the atoms renumbered by a random permutation (meta["perm"][old] = new), the
    bond and angle tables with them; the twin without it has the same geometry (same seed)."""
    molpos, box, rng = _water(nx, ny, nz, seed)
    perm = rng.permutation(3 * len(molpos)) if permute else None
    return _water_system(f"water-{nx}x{ny}x{nz}" + ("-permuted" if permute else ""), molpos, box, perm)


def water_slab(nx, ny, nz, seed):
    """water_box(nx, ny, nz, seed) without the molecules whose oxygen lies in the upper half of the box in z: half the cells
    are empty (but for the hydrogens that reach across), and the density steps from liquid to nothing at two interfaces."""
    molpos, box, _ = _water(nx, ny, nz, seed)
    keep = molpos[:, 0, 2] < 0.5 * box[2]
    return _water_system(f"slab-{nx}x{ny}x{nz}", molpos[keep], box)


def two_clusters(n_each, separation, seed=0, density=0.0213, jitter=0.3):
    """Two argon droplets of n_each atoms (a jittered simple-cubic lattice at liquid density, the n_each sites nearest a
    centre) whose centres lie `separation` apart along x, in an open box (box = 0).  The second droplet is the first one
    turned by a quarter about x, so that y and z extents differ."""
    rng = np.random.default_rng(seed)
    a = (1.0 / density) ** (1.0 / 3.0)
    k = int(np.ceil((n_each / density * 3 / (4 * np.pi)) ** (1 / 3) / a)) + 2
    g = np.arange(-k, k + 1)
    sites = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3) * a
    centre = np.array([0.31, 0.17, 0.23]) * a
    near = np.argsort(np.linalg.norm(sites - centre, axis=1), kind="stable")[:n_each]
    drop = sites[near] + rng.uniform(-jitter, jitter, size=(n_each, 3))
    second = drop[:, [0, 2, 1]] * np.array([1.0, -1.0, 1.0]) + rng.uniform(-0.05, 0.05, size=(n_each, 3))
    pos = np.concatenate([drop, second + np.array([separation, 0.0, 0.0])])
    n = len(pos)
    mol = Topology(atomtype=np.full(n, "AR", dtype=object), charge=np.zeros(n, dtype=np.float32), masses=np.full(n, 39.95, dtype=np.float32))
    return ListSystem(f"clusters-{n_each}", mol, pos, np.zeros(3), "argon")


CLUSTERS = dict(n_each=1700, separation=10500.0)  # the planner takes m = 1 at this density: 1 024 x 5 x 5 cells of >= 10.2 A


def skin_weights(n, seed):
    """Weights in [0.3, 1], one of them exactly 1 (it sets rlist = cutoff + skin) and a single smallest one."""
    rng = np.random.default_rng(seed)
    w = rng.uniform(0.3, 1.0, size=n)
    w[rng.integers(n)] = 1.0
    lo = int(np.argmin(w))
    w[lo] = 0.3  # (the draw is > 0.3 everywhere else: the smallest weight is unique)
    return w


def half_skins(w, dtype_is_f32, skin=SKIN):
    """The library's half skins for weights w with TMDHIP_VSKIN=0: 0.5 skin w_i, rounded to the context's type"""
    h = 0.5 * skin * np.asarray(w, dtype=np.float64)
    return h.astype(np.float32).astype(np.float64) if dtype_is_f32 else h


def displaced(pos, half_skin, seed, fraction=0.98):
    """Every atom moved by `fraction` of its half skin in a random direction (fp64)."""
    rng = np.random.default_rng(seed)
    v = rng.normal(size=pos.shape)
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return pos + v * (fraction * np.asarray(half_skin))[:, None]


def one_atom_beyond(ref, moved, half_skin, atom, seed, fraction=1.02):
    """`moved` with the one atom `atom` put `fraction` of its half skin away from its position in `ref`."""
    rng = np.random.default_rng(seed)
    v = rng.normal(size=3)
    out = moved.copy()
    out[atom] = ref[atom] + v / np.linalg.norm(v) * fraction * half_skin[atom]
    return out


def round_to(pos, dtype_is_f32):
    """Positions as a context of that precision receives them (float64 again)"""
    return pos.astype(np.float32).astype(np.float64) if dtype_is_f32 else pos
