"""Oracle checks of systems too large for a dense evaluation (helpers of the GPU tests).

- `sample_forces`: the forces on k randomly picked atoms, complete (every candidate pair that touches one of them goes
  through `orc.compute`), for a periodic box;
- `periodic_count`: the whole-box in-cutoff pair count by the oracle's decision arithmetic (`orc.pair_geometry`, minimum
  image, `dist <= cutoff`, in the positions' precision), in chunks;
- `open_count`: the same decision on explicit positions without minimum image (a brick of the domain decomposition: own
  rows, then halo rows that are images already), split into own-own and own-halo pairs;
- `shell_count`: the pairs whose minimum-image distance lies within `eps` of the cutoff (float64 geometry).

Everything is chunked so that 10^6 atoms (3.3e7 pairs) fit in memory."""

import numpy as np
import torch

CHUNK = 4_000_000


def _wrap(p64, box):
    w = p64 - np.floor(p64 / box) * box
    return np.where(w >= box, w - box, w)


def periodic_tree(pos, box):
    """cKDTree of the wrapped positions (`pos` [N, 3], any float type) in the periodic box `box` [3]."""
    from scipy.spatial import cKDTree

    b = np.asarray(box, dtype=np.float64)
    return cKDTree(_wrap(np.asarray(pos, dtype=np.float64), b), boxsize=b)


def sample_pairs(tree, n, k, seed, rlist, extra=None):
    """k atoms picked at random (plus the atoms `extra`, sorted, unique) and every candidate pair (minimum image <= rlist)
    that touches one of them: [P, 2] int64, i < j, sorted (i asc, j asc) like the oracle's dense list."""
    pick = np.sort(np.random.default_rng(seed).choice(n, k, replace=False))
    if extra is not None:
        pick = np.union1d(pick, np.asarray(extra, dtype=np.int64))
    nb = tree.query_ball_point(tree.data[pick], rlist, workers=-1)
    i = np.repeat(pick, [len(x) for x in nb])
    j = np.concatenate([np.asarray(x, dtype=np.int64) for x in nb])
    keep = i != j
    lo, hi = np.minimum(i[keep], j[keep]), np.maximum(i[keep], j[keep])
    key = np.unique(lo * np.int64(n) + hi)  # pairs between two picked atoms were found twice
    return pick, np.stack([key // n, key % n], axis=1)


def sample_forces(par, pos, box, terms, k, seed, rlist=9.5, tree=None, extra=None, **kw):
    """Oracle forces on k picked atoms of one replica.  `pos` [1, N, 3], `box` [1, 3, 3] (CPU tensors).
    Returns (pick, forces [k, 3] on the picked atoms, number of candidate pairs, in-cutoff pairs among them)."""
    from oracle import torchmd_oracle as orc

    n = pos.shape[1]
    b = box[0].diagonal().double().numpy()
    if tree is None:
        tree = periodic_tree(pos[0].double().numpy(), b)
    pick, pairs = sample_pairs(tree, n, k, seed, rlist, extra)
    _, F, nin = orc.compute(par, pos, box, terms, pairs=pairs, **kw)
    return pick, F[0, pick], len(pairs), nin[0]


def periodic_count(pos, box, cutoff, tree=None, margin=0.05):
    """In-cutoff pairs of the whole periodic box by the oracle's arithmetic (`pos` [N, 3] tensor in the precision of the
    engine; `box` [3]): candidates from the tree (float64, cutoff + margin), decision `pair_geometry` + `d <= cutoff`."""
    from oracle import torchmd_oracle as orc

    if tree is None:
        tree = periodic_tree(pos.double().numpy(), box)
    allp = tree.query_pairs(cutoff + margin, output_type="ndarray")
    bt = torch.as_tensor(np.asarray(box, dtype=np.float64)).to(pos.dtype)
    total = 0
    for c in range(0, len(allp), CHUNK):
        idx = torch.as_tensor(allp[c: c + CHUNK].astype(np.int64))
        d, _, _ = orc.pair_geometry(pos, idx, bt)
        total += int((d <= cutoff).sum().item())
    return total


def open_count(pos, nown, cutoff, margin=0.05):
    """In-cutoff pairs of explicit positions `pos` [n, 3] (a brick's own rows followed by its halo rows, in the engine's
    precision) that touch an owned row (< nown), by the brick's criterion: the plain difference of the stored
    coordinates (no minimum image), `pair_geometry` with a zero box + `d <= cutoff`.  Returns (own-own, own-halo)."""
    from scipy.spatial import cKDTree

    from oracle import torchmd_oracle as orc

    tree = cKDTree(pos.double().numpy())
    allp = tree.query_pairs(cutoff + margin, output_type="ndarray")
    allp = allp[(allp[:, 0] < nown) | (allp[:, 1] < nown)]  # (halo-halo pairs belong to other bricks)
    oo = oh = 0
    for c in range(0, len(allp), CHUNK):
        part = allp[c: c + CHUNK].astype(np.int64)
        d, _, _ = orc.pair_geometry(pos, torch.as_tensor(part), None)
        inside = (d <= cutoff).numpy()
        both = (part[:, 0] < nown) & (part[:, 1] < nown)
        oo += int((inside & both).sum())
        oh += int((inside & ~both).sum())
    return oo, oh


def shell_count(pos, box, cutoff, eps, tree=None):
    """Pairs with |r - cutoff| <= eps (minimum image, float64): the pairs whose in/out decision may flip when the same
    atoms are stored as other fp32 images."""
    if tree is None:
        tree = periodic_tree(np.asarray(pos, dtype=np.float64), box)
    return int(tree.count_neighbors(tree, cutoff + eps) - tree.count_neighbors(tree, cutoff - eps)) // 2


def mixed_system(nside, dtype, seed=12, a=3.6):
    """A Lennard-Jones + reaction-field mixture on a jittered lattice: three atom types of which two share their LJ
    parameters (the engine merges them into one class, so the type -> class map is exercised), different masses and
    charges.  Returns (Topology, pos [N, 3], box [3], Parameters, terms)."""
    from torchmd_amd.builders import Topology
    from torchmd_amd.forcefields.ff_yaml import YamlForceField
    from torchmd_amd.parameters import Parameters

    rng = np.random.default_rng(seed)
    g = np.arange(nside)
    sites = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float64)
    pos = sites * a + a / 2 + rng.uniform(-0.3, 0.3, size=sites.shape)
    n = len(pos)
    box = np.array([nside * a] * 3)
    kinds = np.array(["A1", "A2", "B"], dtype=object)[rng.integers(0, 3, size=n)]
    ff = {
        "atomtypes": ["A1", "A2", "B"],
        "lj": {"A1": {"sigma": 3.345, "epsilon": 0.238}, "A2": {"sigma": 3.345, "epsilon": 0.238}, "B": {"sigma": 3.0, "epsilon": 0.15}},
        "electrostatics": {"A1": {"charge": 0.1}, "A2": {"charge": -0.1}, "B": {"charge": 0.0}},
        "masses": {"A1": 39.95, "A2": 20.0, "B": 30.0},
    }
    charge = np.array([ff["electrostatics"][k]["charge"] for k in kinds], dtype=np.float32)
    masses = np.array([ff["masses"][k] for k in kinds], dtype=np.float32)
    mol = Topology(atomtype=kinds, charge=charge, masses=masses)
    terms = ["lj", "electrostatics"]
    return mol, pos, box, Parameters(YamlForceField(mol, ff), mol, terms, precision=dtype), terms
