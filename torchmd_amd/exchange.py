"""Temperature replica exchange on the ladder of a `VelocityRescale` thermostat.

`ReplicaExchange(frequency=500, seed=None)`, handed to `Integrator(..., thermostat=VelocityRescale(<ladder>), exchange=...)`,
attempts every `frequency` steps to swap the temperatures of replicas on neighbouring rungs of the ladder (Sugita & Okamoto,
Chem. Phys. Lett. 314, 141, 1999).  Temperatures are swapped, not configurations: a replica slot keeps its positions, box,
neighbour lists and engine state, and two slots trade rungs.  One attempt, number k over the object's life:

1. parity = k mod 2; the pairs of rungs (a, a + 1) for a = parity, parity + 2, ... < R - 1 are tried; slots i and j hold them;
2. Delta = (1 / k_B T_a - 1 / k_B T_{a+1}) (U_i - U_j) with the potential energies the last segment returned; the swap is
   accepted when Delta >= 0 or u < exp(Delta) — the decision is made on the host, where the energies already are;
3. `thermostat.temperatures` is permuted in place, so that slot i holds the temperature of its new rung (the thermostat's
   random streams stay with the slot);
4. the velocities of every slot are scaled by sqrt(T_new / T_old) — exactly 1.0, and then not written, for a slot that keeps
   its rung — by `tmdhip_velocity_rescale` (exchange.hip), one pair of launches for up to 16 replicas, which also records
   the kinetic energy before and after and accumulates their difference (`work()`).

No list is invalidated and nothing is copied between slots.  With exchange, E_kin + E_pot - heat - work is the conserved
quantity of a slot (`heat` the thermostat's).

Random numbers: one `numpy.random.Generator(Philox(key=(seed, 0)))`, exactly one `.random()` per tried pair, in rung order,
drawn whether or not the decision needs it, so the stream position depends on the number of attempts only.
"""

from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _lib as L
from .controls import Control, philox_stream, require_layout, whole_frequency
from .integrator import BOLTZMAN


def temperature_ladder(tmin, tmax, n):
    """A geometric ladder of `n` temperatures from `tmin` to `tmax` (both ends exact): T_a = tmin (tmax / tmin)^(a / (n - 1)),
    the spacing that gives equal acceptance between all neighbours of a system with a constant heat capacity."""
    if int(n) != n or n < 1:
        raise ValueError("a ladder has a positive number of rungs")
    n = int(n)
    if not (np.isfinite(tmin) and np.isfinite(tmax) and 0 < tmin and (tmin < tmax if n > 1 else tmin <= tmax)):
        raise ValueError("a ladder needs 0 < tmin < tmax")
    if n == 1:
        return np.array([float(tmin)])
    t = float(tmin) * (float(tmax) / float(tmin)) ** (np.arange(n) / (n - 1))
    t[0], t[-1] = float(tmin), float(tmax)
    return t


def exchange_decisions(U, temperatures_of_rung, rung_of_slot, parity, u):
    """The swaps of one attempt.  `U` [R]: potential energy per slot; `temperatures_of_rung` [R]: the ladder; `rung_of_slot`
    [R]: the rung each slot holds (a permutation); `parity`: 0 or 1; `u`: one uniform number in [0, 1) per tried pair, in rung
    order.  Returns (new rung_of_slot [R], accepted [npairs] bool, Delta [npairs], pairs [npairs, 2] = the rungs (a, a + 1))."""
    U = np.asarray(U, dtype=np.float64).reshape(-1)
    T = np.asarray(temperatures_of_rung, dtype=np.float64).reshape(-1)
    rungs = np.array(rung_of_slot, dtype=np.int64).reshape(-1)
    R = len(rungs)
    if len(U) != R or len(T) != R or not np.array_equal(np.sort(rungs), np.arange(R)):
        raise ValueError("U, temperatures_of_rung and rung_of_slot need one entry per replica, rung_of_slot a permutation")
    pairs = np.array([(a, a + 1) for a in range(int(parity) % 2, R - 1, 2)], dtype=np.int64).reshape(-1, 2)
    u = np.asarray(u, dtype=np.float64).reshape(-1)
    if len(u) != len(pairs):
        raise ValueError(f"{len(pairs)} pairs are tried: u needs as many entries, has {len(u)}")
    slot_of_rung = np.argsort(rungs)
    accepted = np.zeros(len(pairs), dtype=bool)
    delta = np.zeros(len(pairs))
    for k, (a, b) in enumerate(pairs):
        i, j = slot_of_rung[a], slot_of_rung[b]
        delta[k] = (1.0 / (BOLTZMAN * T[a]) - 1.0 / (BOLTZMAN * T[b])) * (U[i] - U[j])
        accepted[k] = bool(delta[k] >= 0.0 or u[k] < math.exp(delta[k]))  # (NaN energies reject)
        if accepted[k]:
            rungs[i], rungs[j] = b, a
    return rungs, accepted, delta, pairs


class ReplicaExchange(Control):
    """Temperature replica exchange; see the module docstring.  `attempt(system, masses, thermostat, epot)` is what the
    integrator calls every `frequency` steps.  `rungs`: host int array [R], the rung held by each slot; `attempts` /
    `accepted`: int64 [R - 1], per pair of neighbouring rungs; `record`: the last attempt's `pairs`, `U`, `delta`, `u`,
    `accepted`, `rungs` and `factors`; `history`: `rungs.copy()` after every attempt; `last`: the device record of the last
    attempt, double [R, 5] = {K_before, factor, K_after, work, applications}; `work()`: the sum of K_after - K_before over all
    attempts, per slot; `rng`: the generator (anything with `.random()`)."""

    rank = 2

    def __init__(self, frequency=500, seed=None):
        if isinstance(frequency, bool) or not isinstance(frequency, (int, float, np.integer, np.floating)):
            frequency = 0  # (refused below)
        super().__init__(frequency, seed, "frequency must be a positive whole number of steps")
        self.rng = philox_stream(self.seed, 0)
        self.ladder = None  # temperature of every rung, taken from the thermostat at the first attempt
        self.rungs = None
        self.attempts = self.accepted = None
        self.nattempts = 0
        self.record = None
        self.history = []

    def attach(self, integrator):
        """What is refused (ValueError): atom groups, a barostat (which knows one temperature), and what `check` refuses."""
        it = integrator
        if it.batch is not None:
            raise ValueError("exchange= does not support atom groups (batch=): a replica slot is rescaled as a whole")
        if it.barostat is not None:
            raise ValueError("exchange= cannot run under barostat=: the barostat holds one temperature")
        whole_frequency(self.frequency, "the exchange frequency must be a positive whole number of steps")
        self.check(it.thermostat, it.systems.pos.shape[0])

    def after_segment(self, integrator, out):
        """Attempted with the potential energies the segment returned: positions have not moved since."""
        it = integrator
        self.attempt(it.systems, it.masses, it.thermostat, out[1])
        it.kinetic_source = self
        return out

    def kinetic(self):
        return self.last[:, L.EXCHANGE_K_AFTER]

    @staticmethod
    def check(thermostat, nreplicas):
        """What is refused (ValueError): a thermostat that is no `VelocityRescale` holding a sequence of temperatures, one
        entry per replica, strictly increasing."""
        from .thermostat import VelocityRescale

        if not isinstance(thermostat, VelocityRescale) or not thermostat.ladder:
            raise ValueError("exchange= needs thermostat=VelocityRescale(<sequence of temperatures>): a temperature ladder with "
                             "one rung per replica (Langevin's friction is shared by all replicas and cannot carry one)")
        t = thermostat.targets(nreplicas)
        if not (np.diff(t) > 0).all():
            raise ValueError("exchange= needs a ladder of strictly increasing temperatures")

    def bind(self, thermostat, nreplicas):
        """Take the ladder from the thermostat (at the first attempt: slot r holds rung r) and check that both still match."""
        R = int(nreplicas)
        if self.rungs is None:
            self.check(thermostat, R)
            self.ladder = np.array(thermostat.temperatures, dtype=np.float64)
            self.rungs = np.arange(R, dtype=np.int64)
            self.attempts = np.zeros(R - 1, dtype=np.int64)
            self.accepted = np.zeros(R - 1, dtype=np.int64)
        if len(self.rungs) != R or len(thermostat.temperatures) != R:
            raise RuntimeError(f"the exchange holds {len(self.rungs)} rungs for {R} replicas")

    def decide(self, epot):
        """The host half of an attempt: draw one number per tried pair and decide.  Changes nothing but the random stream;
        returns (rungs, accepted, delta, pairs, u) for the attempt that `attempts so far` makes next."""
        parity = self.nattempts % 2
        ntried = len(range(parity, len(self.rungs) - 1, 2))
        u = np.array([self.rng.random() for _ in range(ntried)], dtype=np.float64)
        return exchange_decisions(epot, self.ladder, self.rungs, parity, u) + (u,)

    def attempt(self, system, masses, thermostat, epot):
        """One attempt: decide on the host from `epot` [R] (the potential energies of the slots as they are), permute
        `thermostat.temperatures` in place, and enqueue the rescaling of `system.vel` [R, N, 3] on the current stream (no
        host synchronisation).  Returns (and keeps as `.record`) the record of the attempt."""
        vel = system.vel
        R, N = require_layout(vel, "system.vel", masses)
        U = np.asarray(epot, dtype=np.float64).reshape(-1)
        if len(U) != R:
            raise ValueError(f"epot holds {len(U)} energies for {R} replicas")
        self.bind(thermostat, R)
        self._workspace("tmdhip_velocity_rescale_workspace", R, vel.device)
        rungs, accepted, delta, pairs, u = self.decide(U)
        t_old = np.array(thermostat.temperatures, dtype=np.float64)
        t_new = self.ladder[rungs]
        factors = np.ones(R)
        moved = rungs != self.rungs
        factors[moved] = np.sqrt(t_new[moved] / t_old[moved])
        thermostat.temperatures[:] = t_new
        with torch.cuda.device(vel.device):
            L.check(
                L.load().tmdhip_velocity_rescale(
                    L.dtype_code(vel.dtype), R, N, vel.data_ptr(), masses.data_ptr(), factors.ctypes.data_as(C.POINTER(C.c_double)),
                    self._record.data_ptr(), self._partials.data_ptr(),
                    C.c_void_p(torch.cuda.current_stream(vel.device).cuda_stream),
                ),
                "tmdhip_velocity_rescale",
            )
        self.rungs = rungs
        self.attempts[pairs[:, 0]] += 1
        self.accepted[pairs[accepted, 0]] += 1
        self.nattempts += 1
        self.history.append(rungs.copy())
        self.record = {"pairs": pairs, "U": U.copy(), "delta": delta, "u": u, "accepted": accepted, "rungs": rungs.copy(),
                       "factors": factors}
        return self.record

    @property
    def last(self):
        """Device record of the last attempt, double [R, 5]: K_before, factor, K_after, work, applications (None before the
        first)."""
        return self._record

    def work(self):
        """Energy the rescalings have put into each slot so far (sum of K_after - K_before), host array [R]; synchronises."""
        if self._record is None:
            return None
        return self._record[:, L.EXCHANGE_WORK].cpu().numpy().copy()
