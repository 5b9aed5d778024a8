"""Models for the Hamiltonian exchange, written independently of torchmd_amd/hrex.py: the Metropolis decision
pair by pair, a side term of 1-D harmonic windows that lives on the host (so that the control can be driven without a GPU and
against an acceptance rate known in closed form), and the by-hand permutation of a term's per-replica tables."""

import math

import numpy as np

from torchmd_amd._lib import SideTerm

BOLTZMAN = 0.001987191


def pairs_of(parity, R):
    return [(a, a + 1) for a in range(parity % 2, R - 1, 2)]


def decide(M, states, parity, u, beta):
    """The swaps of one attempt: (new states, accepted, delta), one entry of `u` per tried pair in state order.  Slots i and j
    hold the states a and a + 1; the swap puts i into a + 1 and j into a."""
    states = [int(s) for s in states]
    acc, delta = [], []
    for k, (a, b) in enumerate(pairs_of(parity, len(states))):
        i, j = states.index(a), states.index(b)
        before = M[i][a] + M[j][b]
        after = M[i][b] + M[j][a]
        d = -beta * (after - before)
        ok = (d >= 0.0) or (u[k] < math.exp(d))  # (a NaN fails both comparisons)
        if ok:
            states[i], states[j] = b, a
        acc.append(bool(ok)), delta.append(d)
    return np.array(states, dtype=np.int64), np.array(acc, dtype=bool), np.array(delta, dtype=np.float64)


def acceptance_of_two_windows(beta, k, d):
    """Two harmonic windows k (x - c)^2 / 2 with centres d apart, each slot in equilibrium in its own window: the exact
    acceptance of the swap.  x_i - c_a and x_j - c_b are independent normals of variance 1 / (beta k); Delta =
    -beta k d (d - z) with z = (x_j - c_b) - (x_i - c_a) of variance 2 / (beta k), and E[min(1, exp(Delta))] =
    erfc(sqrt(beta k) d / 2)."""
    return math.erfc(math.sqrt(beta * k) * d / 2.0)


class Windows(SideTerm):
    """R harmonic windows on the x coordinate of atom 0 of every replica: U_a(x) = k (x - c_a)^2 / 2.  Everything on the host:
    `cross_energies` reads `pos[:, 0, 0]` of a CPU tensor."""

    side_name, side_width = "windows", 1

    def __init__(self, centres, k):
        self.centres = np.array(centres, dtype=np.float64)
        self.k = float(k)
        self.version = 0
        self.assigned = []  # every state_of_slot that was assigned

    def exchange_parameters(self, nreplicas):
        if len(self.centres) != nreplicas:
            raise ValueError(f"{len(self.centres)} windows for {nreplicas} replicas")
        return self.centres.copy()

    def cross_energies(self, owner, pos, box, snapshot):
        x = pos[:, 0, 0].detach().cpu().double().numpy()
        return 0.5 * self.k * (x[:, None] - np.asarray(snapshot)[None, :]) ** 2

    def assign_states(self, snapshot, state_of_slot):
        self.centres = np.asarray(snapshot)[np.asarray(state_of_slot)].copy()
        self.version += 1
        self.assigned.append([int(s) for s in state_of_slot])


class Constant(SideTerm):
    """A term that hands out a fixed matrix (slot, state) and records its assignments."""

    side_name, side_width = "constant", 1

    def __init__(self, M):
        self.M = np.array(M, dtype=np.float64)
        self.version = 0
        self.assigned = []

    def exchange_parameters(self, nreplicas):
        return np.arange(len(self.M))

    def cross_energies(self, owner, pos, box, snapshot):
        return self.M.copy()

    def assign_states(self, snapshot, state_of_slot):
        self.version += 1
        self.assigned.append([int(s) for s in state_of_slot])


def states_case(R, nrows, seed=0):
    """R replicas, exactly `nrows` restrained atoms among nrows + 40, a box of its own per replica with the z axis open, k and
    r0 distinct per replica.  A third of the atoms are position-restrained (some references a box away), the others are paired
    into distance restraints; with four rows or more there are three further pairs between restrained atoms (an atom in several
    entries), the first pair is coincident, and about a tenth of the entries of every replica has k = 0.
    Returns (pos [R,N,3], boxes [R,3], mass [N], Restraints)."""
    from torchmd_amd.restraints import Restraints

    rng = np.random.default_rng(1000 * R + nrows + seed)
    N = nrows + 40
    boxes = np.stack([np.array([20.0 + 0.5 * r, 21.0 + 0.25 * r, 0.0]) for r in range(R)])
    pos = rng.uniform(0.0, 20.0, (R, N, 3))
    mass = np.where(rng.random(N) < 0.6, 1.008, 15.999)
    pick = rng.choice(N, nrows, replace=False)
    npos = max(1, nrows // 3)
    rest = pick[npos:]
    if len(rest) % 2:
        rest = np.concatenate([rest, pick[:1]])  # (the odd one pairs with a position-restrained atom)
    pairs = rest.reshape(-1, 2)
    if nrows >= 4:
        pairs = np.concatenate([pairs, np.array([[pick[0], pick[-1]], [pick[-1], pick[1]], [pick[2], pick[-1]]])])
    rs = Restraints(R)
    ref = pos[:, pick[:npos]] + rng.normal(0.0, 0.7, (R, npos, 3))
    ref[:, 0, 0] += boxes[:, 0]  # the same point one box further
    ref[:, 0, 2] += 3.0  # (the open axis: no image)
    kp = rng.uniform(1.0, 120.0, (R, npos))
    kp[rng.random((R, npos)) < 0.1] = 0.0
    rs.add_position(pick[:npos], ref, kp)
    if len(pairs):
        pos[:, pairs[0, 1]] = pos[:, pairs[0, 0]]  # a coincident pair: r = 0
        if len(pairs) > 1:
            pos[:, pairs[1, 0], 0], pos[:, pairs[1, 1], 0] = 0.3, 19.6  # a pair across a face
        kd = rng.uniform(1.0, 150.0, (R, len(pairs)))
        kd[rng.random((R, len(pairs))) < 0.1] = 0.0
        kd[:, 0] = rng.uniform(1.0, 150.0, R)  # (the coincident pair counts in every replica)
        rs.add_distance(pairs, rng.uniform(0.5, 6.0, (R, len(pairs))), kd)
    assert len(rs.atoms()) == nrows
    return pos, boxes, mass, rs


def cross_model(rs, pos, boxes):
    """[R, R, 2]: entry [i, k] = the (position, distance) energy of configuration i in box i under row k of the tables, from
    `Restraints.energy_forces` with the rows of the tables rotated (shift s puts row (i + s) mod R in front of configuration i)."""
    from torchmd_amd.restraints import Restraints

    R = rs.nreplicas
    out = np.zeros((R, R, 2))
    for s in range(R):
        rows = (np.arange(R) + s) % R
        m = Restraints(R)
        if rs.npos:
            m.add_position(rs.pos_atom, rs.pos_ref[rows], rs.pos_k[rows])
        if rs.ndist:
            m.add_distance(rs.dist_pair, rs.dist_r0[rows], rs.dist_k[rows])
        E = m.energy_forces(pos, boxes)[0]
        out[np.arange(R), rows] = E
    return out


class BarePar:
    """What `Forces(terms=[])` asks of its parameters: a context with atoms and no force term of its own."""

    def __init__(self, mass, dtype):
        import torch

        self.masses = torch.tensor(mass, dtype=dtype)
        self.charges = torch.zeros(len(mass), dtype=dtype)
        self.nonbonded_params = None
        self.bond_params = self.angle_params = self.dihedral_params = self.improper_params = self.nonbonded_14_params = None
        self.mapped_atom_types = torch.zeros(len(mass), dtype=torch.int64)
        self.natoms = len(mass)

    def get_exclusions(self, types=("bonds", "angles", "1-4"), fullarray=False):
        return []


def permute_restraints(rs, tables0, state_of_slot):
    """What the tables of a `Restraints` are when slot r holds state `state_of_slot[r]` of `tables0` = (pos_ref, pos_k,
    dist_r0, dist_k) — row by row, by hand."""
    out = [np.empty_like(t) for t in tables0]
    for r, a in enumerate(state_of_slot):
        for dst, src in zip(out, tables0):
            dst[r] = src[a]
    return out
