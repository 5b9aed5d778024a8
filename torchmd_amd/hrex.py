"""Hamiltonian replica exchange: replicas trade alchemical couplings and umbrella windows.

`HamiltonianExchange(frequency=500, temperature=None, seed=None, keep_matrices=False)`, handed to
`Integrator(..., exchange=...)`, attempts every `frequency` steps to swap the per-replica parameters of the force terms that
have some — the couplings of an `Alchemical`, the references, targets and strengths of a `Restraints` — between replicas that
hold neighbouring states (lambda-exchange; replica-exchange umbrella sampling, Sugita, Kitao & Okamoto, J. Chem. Phys. 113,
6042, 2000).  All replicas run at one temperature.  Parameters are swapped, not configurations (§16's rule): a replica slot
keeps its positions, box, neighbour lists and engine state, and two slots trade states.  State a is row a of the parameters
as they were when the integrator was made; slot r starts in state r.  One attempt, number n over the object's life:

1. every exchangeable term gives its cross energies, M[r][a] = the term's potential of slot r's configuration under state a
   (`SideTerm.cross_energies`: tmdhip_alchemical_states, tmdhip_restraint_states); M is their sum, on the host;
2. parity = n mod 2; the pairs of states (a, a + 1) for a = parity, parity + 2, ... < R - 1 are tried; slots i and j hold them;
3. Delta = -beta [(M[i][a+1] + M[j][a]) - (M[i][a] + M[j][a+1])]; the swap is accepted when Delta >= 0 or u < exp(Delta);
4. if a slot moved: every term is given the new assignment (`SideTerm.assign_states`) and `forces.compute` runs once, so that
   `systems.forces` and the potential energies the call returns are those of the new Hamiltonians — the next step's first
   half-kick uses them.  Velocities are never touched.  If nothing moved nothing further is launched.

The energy a slot gains when its Hamiltonian is replaced under it, U_new(x) - U_old(x) = M[r][new] - M[r][old], is accumulated
(`work()`): E_kin + E_pot - work is the conserved quantity of a slot in an NVE run.

Random numbers: one `numpy.random.Generator(Philox(key=(seed, 0)))`, exactly one `.random()` per tried pair, in state order,
drawn whether or not the decision needs it, so the stream position depends on the number of attempts only.
"""

from __future__ import annotations

import math

import numpy as np

from .controls import Control, philox_stream, whole_frequency
from .forces import active_side_terms
from .integrator import BOLTZMAN


def hamiltonian_decisions(M, state_of_slot, parity, u, beta):
    """The swaps of one attempt.  `M` [R, R]: M[r][a] = potential of slot r's configuration under state a (a constant per row
    does not matter); `state_of_slot` [R]: the state each slot holds (a permutation); `parity`: 0 or 1; `u`: one uniform number
    in [0, 1) per tried pair, in state order; `beta` = 1 / k_B T.  Returns (new state_of_slot [R], accepted [npairs] bool,
    Delta [npairs], pairs [npairs, 2] = the states (a, a + 1))."""
    states = np.array(state_of_slot, dtype=np.int64).reshape(-1)
    R = len(states)
    M = np.asarray(M, dtype=np.float64)
    if M.shape != (R, R) or not np.array_equal(np.sort(states), np.arange(R)):
        raise ValueError("M must be [R, R] and state_of_slot a permutation of the R states")
    pairs = np.array([(a, a + 1) for a in range(int(parity) % 2, R - 1, 2)], dtype=np.int64).reshape(-1, 2)
    u = np.asarray(u, dtype=np.float64).reshape(-1)
    if len(u) != len(pairs):
        raise ValueError(f"{len(pairs)} pairs are tried: u needs as many entries, has {len(u)}")
    slot_of_state = np.argsort(states)
    accepted = np.zeros(len(pairs), dtype=bool)
    delta = np.zeros(len(pairs))
    for k, (a, b) in enumerate(pairs):
        i, j = slot_of_state[a], slot_of_state[b]
        delta[k] = -float(beta) * ((M[i, b] + M[j, a]) - (M[i, a] + M[j, b]))
        accepted[k] = bool(delta[k] >= 0.0 or u[k] < math.exp(delta[k]))  # (NaN energies reject)
        if accepted[k]:
            states[i], states[j] = b, a
    return states, accepted, delta, pairs


class HamiltonianExchange(Control):
    """Hamiltonian replica exchange; see the module docstring.  `attempt(system, forces, epot)` is what the integrator calls
    every `frequency` steps.  `states`: host int array [R], the state held by each slot; `attempts` / `accepted`: int64
    [R - 1], per pair of neighbouring states; `record`: the last attempt's `pairs`, `M`, `delta`, `u`, `accepted` and `states`;
    `history`: `states.copy()` after every attempt; `matrices`: beta M of every attempt with `keep_matrices` (the reduced
    potentials MBAR asks for, [slot, state]); `work()`: per slot, the sum over attempts of U_new(x) - U_old(x); `beta`:
    1 / k_B T; `rng`: the generator (anything with `.random()`)."""

    rank = 2  # (ReplicaExchange's slot, `Integrator(exchange=)`: the two cannot coexist)

    def __init__(self, frequency=500, temperature=None, seed=None, keep_matrices=False):
        if isinstance(frequency, bool) or not isinstance(frequency, (int, float, np.integer, np.floating)):
            frequency = 0  # (refused below)
        super().__init__(frequency, seed, "frequency must be a positive whole number of steps")
        if temperature is not None and not (np.ndim(temperature) == 0 and np.isfinite(temperature) and temperature > 0):
            raise ValueError("temperature must be one positive number: all replicas of a Hamiltonian exchange share it")
        self.temperature = None if temperature is None else float(temperature)
        self.keep_matrices = bool(keep_matrices)
        self.rng = philox_stream(self.seed, 0)
        self.beta = None
        self.terms = self.snapshots = self._versions = None
        self.states = self.attempts = self.accepted = self._work = None
        self.nattempts = 0
        self.record = None
        self.history = []
        self.matrices = []

    # ------------------------------------------------------------------ set-up
    @staticmethod
    def common_temperature(given, integrator):
        """`given`, else Langevin's T, else the one common target of the thermostat (ValueError: a ladder of distinct
        temperatures, or no temperature at all)."""
        if given is not None:
            return float(given)
        if integrator.T:
            return float(integrator.T)
        th = integrator.thermostat
        if th is not None:
            if th.temperature is None:
                raise ValueError("a Hamiltonian exchange needs one temperature for all replicas: the thermostat holds a ladder of "
                                 "distinct temperatures (temperature exchange: ReplicaExchange)")
            return float(th.temperature)
        raise ValueError("a Hamiltonian exchange needs a temperature: give temperature=, a Langevin T or a thermostat")

    def attach(self, integrator):
        """What is refused (ValueError): atom groups, any barostat, a run with no common temperature, forces with no
        exchangeable side term, a term whose parameters are for another number of replicas.  Takes the snapshots: state a is
        row a of the parameters as they are now."""
        it = integrator
        if it.batch is not None:
            raise ValueError("exchange= does not support atom groups (batch=): a replica slot holds one state as a whole")
        if it.barostat is not None:
            raise ValueError("a Hamiltonian exchange cannot run under barostat=: the states would need their volume term")
        whole_frequency(self.frequency, "the exchange frequency must be a positive whole number of steps")
        self.beta = 1.0 / (BOLTZMAN * self.common_temperature(self.temperature, it))
        R = int(it.systems.pos.shape[0])
        found = [(t, t.exchange_parameters(R)) for t in active_side_terms(it.forces)]
        found = [(t, s) for t, s in found if s is not None]
        if not found:
            raise ValueError("a Hamiltonian exchange needs a Forces with a side term that holds parameters per replica "
                             "(alchemical= with one coupling per replica, restraints=)")
        self.terms, self.snapshots = [t for t, _ in found], [s for _, s in found]
        self._versions = [t.version for t in self.terms]
        self.states = np.arange(R, dtype=np.int64)
        self.attempts = np.zeros(max(R - 1, 0), dtype=np.int64)
        self.accepted = np.zeros(max(R - 1, 0), dtype=np.int64)
        self._work = np.zeros(R)

    # ------------------------------------------------------------------ one attempt
    def after_segment(self, integrator, out):
        """Attempted on the state the segment left.  After a swap the potential energies are those of the new assignment;
        the kinetic energies are as they were (`kinetic_source` is left alone)."""
        it = integrator
        pot = self.attempt(it.systems, it.forces, out[1])
        return out if pot is None else (out[0], pot, out[2])

    def cross_matrix(self, system, forces):
        """M [R, R]: the sum of the terms' cross energies at the positions and boxes as they are; host."""
        R = len(self.states)
        M = np.zeros((R, R))
        for t, snap in zip(self.terms, self.snapshots):
            m = np.asarray(t.cross_energies(forces, system.pos, system.box, snap), dtype=np.float64)
            if m.shape != (R, R):
                raise RuntimeError(f"{t.side_name}: cross energies of shape {m.shape} for {R} replicas")
            M += m
        return M

    def decide(self, M):
        """The host half of an attempt: draw one number per tried pair and decide.  Changes nothing but the random stream;
        returns (states, accepted, delta, pairs, u) for the attempt that `nattempts` makes next."""
        parity = self.nattempts % 2
        ntried = len(range(parity, len(self.states) - 1, 2))
        u = np.array([self.rng.random() for _ in range(ntried)], dtype=np.float64)
        return hamiltonian_decisions(M, self.states, parity, u, self.beta) + (u,)

    def attempt(self, system, forces, epot=None):
        """One attempt on `system` (positions and boxes as they are).  Returns the potential energies of the new assignment
        (a list, `forces.compute`'s) when a slot moved — `system.forces` then holds that evaluation's forces — and None when
        nothing moved: then nothing but the cross energies was launched."""
        if self.terms is None:
            raise RuntimeError("the exchange belongs to no integrator yet (Integrator(..., exchange=...))")
        R = int(system.pos.shape[0])
        if R != len(self.states):
            raise RuntimeError(f"the exchange holds {len(self.states)} states for {R} replicas")
        for t, v in zip(self.terms, self._versions):
            if t.version != v:
                raise RuntimeError(f"the {t.side_name} parameters were changed since the exchange last assigned them: its states "
                                   "are rows of the parameters as they were when the integrator was made")
        M = self.cross_matrix(system, forces)
        states, accepted, delta, pairs, u = self.decide(M)
        moved = states != self.states
        pot = None
        if moved.any():
            rows = np.arange(R)
            self._work += M[rows, states] - M[rows, self.states]
            for t, snap in zip(self.terms, self.snapshots):
                t.assign_states(snap, states)
            self._versions = [t.version for t in self.terms]
            self.states = states.copy()
            pot = forces.compute(system.pos, system.box, system.forces)
        self.attempts[pairs[:, 0]] += 1
        self.accepted[pairs[accepted, 0]] += 1
        self.nattempts += 1
        self.history.append(self.states.copy())
        if self.keep_matrices:
            self.matrices.append(self.beta * M)
        self.record = {"pairs": pairs, "M": M, "delta": delta, "u": u, "accepted": accepted, "states": self.states.copy()}
        return pot

    def work(self):
        """Energy the swaps have put into each slot so far (sum of U_new(x) - U_old(x) at the moment of the swap), host [R]."""
        return None if self._work is None else self._work.copy()
